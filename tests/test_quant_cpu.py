"""The device quantisers without a GPU: the third header and its symbol table, every refusal of the four entry points (none
reaches a device), the NumPy restatement (tests/quant_ref.py) against the host quantisers and the reference-written arrays of
both golden fixtures bit for bit, and the Python doors' argument checks."""
import os
import re

import numpy as np
import pytest

import quant_ref
import sparse_rx
from quant_ref import same_bits
from sparse_rx import _capi, dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24]  # never dereferenced
DIMS_LISTED = (1, 3, 31, 48, 65, 200, 768, 1000, 1024)


def test_third_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_quant.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.QUANT_SYMBOLS) and len(declared) == 4, declared ^ set(_capi.QUANT_SYMBOLS)
    assert '#include "sparse_rx.h"' in hdr and "retriever_registry.py:435-462" in hdr
    assert not set(_capi.QUANT_SYMBOLS) & (set(_capi.SYMBOLS) | set(_capi.RESCORE_SYMBOLS))
    assert "dense_quant.hip" in _capi.SOURCES
    assert any(p.endswith("sparse_rx_quant.h") for p in _capi._deps())
    L = _capi.lib()
    for name, (res, args) in _capi.QUANT_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert (_capi.SRX_QUANT_NONFINITE, _capi.SRX_QUANT_DEGENERATE) == (quant_ref.NONFINITE, quant_ref.DEGENERATE) == (1, 2)
    assert re.search(r"#define SRX_QUANT_NONFINITE 1\b", hdr) and re.search(r"#define SRX_QUANT_DEGENERATE 2\b", hdr)
    assert L.srx_version() == 301 and len(_capi.SYMBOLS) == 35  # the frozen parts


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, msg)


def _corpus_refusals(call, name):
    for kw in (dict(n_rows=-1), dict(row0=-32), dict(n_total=-1)):
        _refused(call(**kw), "negative count")
    for kw in (dict(row0=96, n_rows=10), dict(n_rows=101), dict(row0=128)):
        _refused(call(**kw), "row0 + n_rows > n_total")
    for kw in (dict(dim=0), dict(dim=-4), dict(dim=65), dict(dim=1025, dim_pad=1088), dict(ld=47), dict(ld=0)):
        _refused(call(**kw), "dim <= dim_pad <= 1024")
    for null in ("emb", "out", "scales"):
        _refused(call(**{null: None}), "null pointer")
    _refused(call(emb=P[0] + 2), "4-byte aligned")
    for off in (4, 8, 1):
        _refused(call(out=P[1] + off), "16-byte aligned")
    assert call(n_rows=0, emb=None, out=None, scales=None) == 0  # nothing to do: no launch
    assert call(n_rows=0, row0=100) == 0
    _refused(call(n_rows=-1), "negative")
    assert name.encode() in _capi.lib().srx_last_error()  # the text names the entry point


def test_quantize_i8_refusals():
    f = _capi.lib().srx_dense_quantize_i8
    ok = dict(device=0, emb=P[0], ld=48, n_rows=10, dim=48, dim_pad=64, row0=0, n_total=100, packed=0, out=P[1], scales=P[2], flag=None,
              stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    for dim_pad in (48, 160, 640, 80):  # 160 and 640 are multiples of 32 the INT8 engine has no instance for
        _refused(call(dim_pad=dim_pad), "unsupported dim_pad")
    for packed in (2, -1):
        _refused(call(packed=packed), "packed must be")
    for row0 in (1, 31, 33, 48):
        _refused(call(packed=1, row0=row0), "multiple of 32")
    _refused(call(n_rows=1 << 40, n_total=1 << 40), "too many rows")
    assert call(packed=1, row0=64, n_rows=0) == 0
    _corpus_refusals(call, "srx_dense_quantize_i8")


def test_quantize_u8_refusals():
    f = _capi.lib().srx_dense_quantize_u8
    ok = dict(device=0, emb=P[0], ld=48, n_rows=10, dim=48, dim_pad=64, row0=0, n_total=100, out=P[1], scales=P[2], flag=None, stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    for dim_pad in (96, 48, 100):
        _refused(call(dim_pad=dim_pad), "unsupported dim_pad")
    _corpus_refusals(call, "srx_dense_quantize_u8")


def test_quantize_queries_i8_refusals():
    f = _capi.lib().srx_dense_quantize_queries_i8
    ok = dict(device=0, q=P[0], ld=768, nq=5, dim=768, dim_pad=768, out=P[1], scales=P[2], flag=None, stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    _refused(call(nq=-1), "negative count")
    for kw in (dict(dim=0), dict(dim=769), dict(ld=767), dict(dim=1025, dim_pad=1025, ld=1025)):
        _refused(call(**kw), "dim <= dim_pad <= 1024")
    for dim_pad in (800, 832):
        _refused(call(dim_pad=dim_pad), "unsupported dim_pad")
    for null in ("q", "out", "scales"):
        _refused(call(**{null: None}), "null pointer")
    _refused(call(q=P[0] + 1), "4-byte aligned")
    _refused(call(out=P[1] + 8), "16-byte aligned")
    assert call(nq=0, q=None, out=None, scales=None) == 0


def test_quantize_queries_u8_refusals():
    f = _capi.lib().srx_dense_quantize_queries_u8
    ok = dict(device=0, q=P[0], ld=100, nq=5, dim=100, dim_pad=128, out=P[1], scales=P[2], deq=P[3], flag=None, stream=None)
    call = lambda **kw: f(*{**ok, **kw}.values())
    _refused(call(nq=-7), "negative count")
    for kw in (dict(dim=129), dict(ld=99), dict(dim_pad=1088)):
        _refused(call(**kw), "dim <= dim_pad <= 1024")
    for dim_pad in (160, 100):
        _refused(call(dim_pad=dim_pad), "unsupported dim_pad")
    for null in ("q", "deq"):  # the codes and the scale pairs are optional, the de-quantised block is not
        _refused(call(**{null: None}), "null pointer")
    _refused(call(q=P[0] + 3), "4-byte aligned")
    _refused(call(deq=P[3] + 4), "16-byte aligned")
    _refused(call(out=P[1] + 4), "16-byte aligned")
    assert call(nq=0, q=None, deq=None) == 0


# ---- the restatement against the host quantisers and the reference-written arrays ---------------------------------------------
def test_restatement_is_the_reference_on_the_int8_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "dense_int8.npz"))
    emb, qemb = z["emb"], z["qemb"]
    codes, scales, flag = quant_ref.i8_rows(emb)
    host = sparse_rx.quantize_symmetric(emb)
    assert flag == 0 and same_bits(codes, z["corpus_int8"]) and same_bits(scales, z["corpus_scales"])
    assert same_bits(codes, host[0]) and same_bits(scales, host[1])
    qc, qs, flag = quant_ref.i8_queries(qemb)
    assert flag == 0 and same_bits(qc, z["query_int8"]) and same_bits(qs, z["query_scales"].astype(np.float32).reshape(-1))
    for i, e in enumerate(qemb):
        h = sparse_rx.quantize_query_symmetric(e)
        assert same_bits(qc[i], h[0]) and qs[i].view(np.uint32) == np.float32(h[1]).view(np.uint32)
    padded = quant_ref.i8_rows(emb, quant_ref.pad_i8(emb.shape[1]))[0]
    assert padded.shape[1] in quant_ref.DIMS and same_bits(padded[:, : emb.shape[1]], codes) and not padded[:, emb.shape[1]:].any()


def test_restatement_is_the_reference_on_the_uint8_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "dense_int8.npz"))
    a = np.load(os.path.join(golden_dir, "dense_uint8_asym.npz"))
    emb, qemb = z["emb"], z["qemb"]
    codes, table, flag = quant_ref.u8_rows(emb)
    host = sparse_rx.quantize_asymmetric(emb)
    assert flag == 0 and same_bits(codes, a["corpus_uint8"]) and same_bits(table, a["corpus_scales"])
    assert same_bits(codes, host[0]) and same_bits(table, host[1])
    qc, qs, deq, flag = quant_ref.u8_queries(qemb)
    assert flag == 0 and same_bits(qc, a["query_uint8"]) and same_bits(qs, a["query_scales"])
    for i, e in enumerate(qemb):
        h = sparse_rx.quantize_query_asymmetric(e)
        assert same_bits(qc[i], h[0]) and same_bits(qs[i], h[1])
        assert same_bits(deq[i], dense.dequantize_query_asymmetric(h[0], h[1]))


@pytest.mark.parametrize("dim", DIMS_LISTED)
def test_restatement_is_the_host_functions_on_random_rows(dim):
    e = quant_ref.make_rows(dim, 2000, dim)
    with np.errstate(all="ignore"):
        hc, hs = sparse_rx.quantize_symmetric(e)
        uc, ut = sparse_rx.quantize_asymmetric(e)
    codes, scales, flag = quant_ref.i8_rows(e)
    assert flag == 0 and same_bits(codes, hc) and same_bits(scales, hs)
    codes, table, flag = quant_ref.u8_rows(e)
    assert flag == 0 and same_bits(codes, uc) and same_bits(table, ut)
    q = quant_ref.make_rows(dim + 1, 300, dim, degenerate=False, denormal=False)  # queries the reference is defined for
    qc, qs, flag = quant_ref.i8_queries(q)
    uq, us, deq, uflag = quant_ref.u8_queries(q) if dim > 1 else (None, None, None, 0)  # a 1-d query is constant: degenerate
    assert flag == 0 and uflag == 0
    for i in range(0, 300, 7):
        h = sparse_rx.quantize_query_symmetric(q[i])
        assert same_bits(qc[i], h[0]) and qs[i].view(np.uint32) == np.float32(h[1]).view(np.uint32), i
        if dim > 1:
            h = sparse_rx.quantize_query_asymmetric(q[i])
            assert same_bits(uq[i], h[0]) and same_bits(us[i], h[1]) and same_bits(deq[i], dense.dequantize_query_asymmetric(*h)), i


def test_restatement_of_the_defined_edge_cases():
    f = np.float32
    e = np.array([[1, 2, 3, 4], [np.nan, 1, 2, 3], [0, 0, 0, 0], [5, 5, 5, 5], [np.inf, 0, 0, 0], [3e38, -3e38, 0, 0]], f)
    codes, scales, flag = quant_ref.i8_rows(e, 32)
    assert flag == 1 and codes.shape == (6, 32) and not codes[[1, 2, 4]].any() and codes[5].tolist()[:2] == [127, -127]
    assert scales.tolist() == [4.0, f(1e-8), f(1e-8), 5.0, f(1e-8), f(3e38)]  # NaN / inf rows: 1e-8; the zero row: the clamp
    codes, scales, flag = quant_ref.i8_queries(e)
    assert flag == 3 and not codes[[1, 2, 4]].any() and scales[[1, 2, 4]].tolist() == [0, 0, 0] and scales[0] == f(4) / f(127)
    codes, table, flag = quant_ref.u8_rows(e, 64)
    assert flag == 1 and codes.shape == (6, 64) and not codes[[1, 2, 3, 4, 5]].any() and codes[0].tolist()[:4] == [0, 85, 170, 255]
    assert table.tolist() == [f(3) / f(255)] + [f(1e-8)] * 5 + [1, 0, 0, 5, 0, 0]  # 3e38 - -3e38 overflows: flagged, min 0
    codes, pairs, deq, flag = quant_ref.u8_queries(e, 64)
    assert flag == 3 and not codes[1:].any()
    assert pairs.tolist() == [[f(3) / f(255), 1], [0, 0], [0, 0], [0, 5], [0, 0], [0, 0]]
    assert deq[3].tolist() == [5] * 4 + [0] * 60 and not deq[[1, 2, 4, 5]].any()  # a constant query de-quantises to itself
    assert quant_ref.i8_queries(e[[0, 3]])[2] == 0 and quant_ref.u8_queries(e[[0]])[3] == 0 and quant_ref.u8_queries(e[[3]])[3] == 2


def test_unpack_is_the_inverse_of_the_fragment_order():
    import rescore_ref
    rng = np.random.default_rng(4)
    for n, dim in ((33, 32), (70, 96), (5, 1024), (64, 768)):
        rows = rng.integers(-127, 128, (n, dim), dtype=np.int8)
        assert np.array_equal(dense.unpack_i8_host(rescore_ref.pack_i8(rows), n, dim), rows)


# ---- the Python doors -------------------------------------------------------------------------------------------------------
def test_quantize_argument_of_the_doors():
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError, match="quantize"):
            sparse_rx.QuantizedEmbeddingIndex(quantize=bad)
        with pytest.raises(ValueError, match="quantize"):
            sparse_rx.QuantizedEmbeddingRetriever("dpr", "m", quantize=bad)
        with pytest.raises(ValueError, match="quantize"):
            sparse_rx.HybridRetriever(quantize=bad)
    with pytest.raises(ValueError, match="quantize"):
        sparse_rx.RetrieverRegistry.create({"type": "hybrid", "params": {"quantize": "fpga"}})
    assert sparse_rx.QuantizedEmbeddingIndex().quantize == "host"  # the defaults stay
    assert sparse_rx.QuantizedEmbeddingRetriever("dpr", "m").quantize == "host"
    assert sparse_rx.RetrieverRegistry.create({"type": "hybrid"}).dense.quantize == "host"
    assert sparse_rx.RetrieverRegistry.create({"type": "dpr", "params": {"quantize": "device"}}).quantize == "device"
    r = sparse_rx.RetrieverRegistry.create({"type": "hybrid", "params": {"quantize": "Device"}})
    assert r.dense.quantize == "device" and r.dense.corpus_embeddings_int8 is None and r.dense.corpus_scales is None
    r.dense.corpus_scales = np.ones(3, np.float32)  # still plain attributes to a caller
    assert r.dense.corpus_scales.tolist() == [1, 1, 1]


def test_device_quantisers_take_float32_only():
    import torch
    fns = (sparse_rx.quantize_symmetric_device, sparse_rx.quantize_asymmetric_device, sparse_rx.quantize_queries_symmetric_device,
           sparse_rx.quantize_queries_asymmetric_device)
    for fn in fns:
        for x in (torch.zeros((4, 8), dtype=torch.float64), torch.zeros((4, 8), dtype=torch.float16), np.zeros((4, 8), np.float64),
                  torch.zeros((4, 8), dtype=torch.int8)):
            with pytest.raises(ValueError, match="float32"):
                fn(x)
        with pytest.raises(ValueError, match="2-D"):
            fn(torch.zeros(8, dtype=torch.float32))
    for cls in (sparse_rx.DenseInt8Index, sparse_rx.DenseUint8Index):
        with pytest.raises(ValueError, match="float32"):  # checked before the device is looked for
            cls.from_embeddings(np.zeros((4, 8), np.float64))
    with pytest.raises(ValueError, match="float32"):
        dense.stack_queries_f32(None, [np.zeros(8, np.float64)])
