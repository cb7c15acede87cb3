"""The half-precision dense index without a GPU: the fifth header and its symbol table, the frozen counts of the other
four, every refusal of the five entry points (none reaches a device), the two roundings of the NumPy restatement
(tests/half_ref.py) against NumPy's and torch's own, the fragment layout, and the service's storage keyword."""
import ctypes
import os
import re

import numpy as np
import pytest

import half_ref
import sparse_rx
from sparse_rx import _capi
from sparse_rx.dense import DenseHalfIndex, check_half_dtype, unpack_half_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(12)]  # 16-byte aligned addresses, never dereferenced


def test_fifth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_half.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.HALF_SYMBOLS) and len(declared) == 5, declared ^ set(_capi.HALF_SYMBOLS)
    assert '#include "sparse_rx.h"' in hdr and "has no half-precision index" in hdr
    for other in (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS):
        assert not set(_capi.HALF_SYMBOLS) & set(other)
    # the frozen counts: the new entry points are a table of their own, nothing else moved
    assert (len(_capi.SYMBOLS), len(_capi.RESCORE_SYMBOLS), len(_capi.QUANT_SYMBOLS), len(_capi.FILTER_SYMBOLS)) == (35, 4, 4, 8)
    assert "dense_half.hip" in _capi.SOURCES
    deps = [os.path.basename(p) for p in _capi._deps()]
    assert "sparse_rx_half.h" in deps and "half_common.h" in deps and "dense_half.hip" in deps
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.HALF_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert sparse_rx.DenseHalfIndex is DenseHalfIndex and "DenseHalfIndex" in sparse_rx.__all__
    assert (_capi.SRX_HALF_F16, _capi.SRX_HALF_BF16) == (0, 1) == (half_ref.TYPES["f16"], half_ref.TYPES["bf16"])
    assert re.search(r"SRX_HALF_F16 = 0, SRX_HALF_BF16 = 1", hdr)


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, msg)


@pytest.mark.parametrize("n,dim_pad", [(0, 64), (1, 64), (32, 64), (33, 128), (1000, 768), (4099, 1024)])
def test_half_bytes(n, dim_pad):
    assert _capi.lib().srx_dense_half_bytes(n, dim_pad) == half_ref.half_bytes(n, dim_pad)
    if n:
        assert half_ref.byte_offset(n - 1, dim_pad - 1, dim_pad) < half_ref.half_bytes(n, dim_pad)
        assert half_ref.pack(np.zeros((n, dim_pad), np.uint16)).nbytes == half_ref.half_bytes(n, dim_pad)


def test_half_bytes_refusals():
    L = _capi.lib()
    _refused(L.srx_dense_half_bytes(-1, 64), "srx_dense_half_bytes")
    for d in (0, 32, 96, 1088, -64):
        _refused(L.srx_dense_half_bytes(10, d), "dim_pad")


def test_convert_refusals():
    L = _capi.lib()
    ok = dict(device=0, type=0, emb=P[0], ld=100, n_rows=64, dim=100, dim_pad=128, row0=32, n_total=96, out=P[1], flag=None, stream=None)
    call = lambda **kw: L.srx_dense_convert_half(*{**ok, **kw}.values())
    for t in (-1, 2, 7):
        _refused(call(type=t), "type must be")
    for kw in (dict(n_rows=-1), dict(row0=-32), dict(n_total=-1)):
        _refused(call(**kw), "negative count")
    _refused(call(n_total=95), "row0 + n_rows > n_total")
    _refused(call(row0=128, n_total=100, n_rows=0), "row0 + n_rows > n_total")
    for d in (0, 32, 96, 1088):
        _refused(call(dim_pad=d, dim=16, ld=16), "dim_pad")
    for kw in (dict(dim=0), dict(dim=129, ld=200), dict(ld=99)):
        _refused(call(**kw), "dim")
    _refused(call(row0=16, n_total=200), "multiple of 32")
    _refused(call(row0=0, n_rows=2 ** 37, n_total=2 ** 37), "too many rows in one call")  # more than 2^31 - 1 tiles
    _refused(call(row0=0, n_rows=32 * (2 ** 31 - 1) + 1, n_total=2 ** 37), "too many rows in one call")
    assert call(row0=0, n_rows=32 * (2 ** 31 - 1), n_total=2 ** 37, emb=None) == -1 and b"null pointer" in L.srx_last_error()  # the most one call takes
    _refused(call(emb=None), "null pointer")
    _refused(call(out=None), "null pointer")
    _refused(call(emb=P[0] + 2), "4-byte aligned")
    _refused(call(out=P[1] + 8), "16-byte aligned")
    assert b"srx_dense_convert_half" in L.srx_last_error()
    assert call(n_rows=0, emb=None, out=None, n_total=32) == 0  # nothing to do: no launch


def test_workspace_refusals_and_size():
    L = _capi.lib()
    for args in ((-1, 100, 10), (1, 0, 10), (1, 100, 0), (1, 100, 1025)):
        _refused(L.srx_dense_half_workspace_bytes(*args), "srx_dense_half_workspace_bytes")
    # the packed query block (whole tiles of 128, 2 KiB per row) + the score matrix of the pass + the lists of the splits
    small = L.srx_dense_half_workspace_bytes(1, 1000, 10)
    assert small >= 128 * 2048 + 1024 * 4 + 2 * 10 * 4 + 4
    assert L.srx_dense_half_workspace_bytes(2000, 1000, 10) == L.srx_dense_half_workspace_bytes(1024, 1000, 10)  # a pass is <= 1 024 queries
    assert L.srx_dense_half_workspace_bytes(0, 1000, 10) > 0


def _filter(**kw):
    d = dict(bits=P[8], n_filters=1, q_filter=None)
    d.update(kw)
    return ctypes.byref(_capi.DocFilterDesc(**d))


@pytest.mark.parametrize("type_", [0, 1])
def test_search_refusals(type_):
    L = _capi.lib()
    ok = dict(device=0, type=type_, corpus=P[0], n_docs=1000, dim_pad=64, queries=P[2], nq=2, k=10, doc_base=0, filter=None, out_doc=P[3],
              out_score=P[4], out_count=P[5], ws=P[6], ws_bytes=1 << 30, stream=None, offset=0.0)
    call = lambda **kw: L.srx_dense_search_half(*{**ok, **kw}.values())
    for t in (-1, 2):
        _refused(call(type=t), "type must be")
    _refused(call(filter=_filter(bits=None)), "null filter bits")
    _refused(call(filter=_filter(bits=P[8] + 8)), "16-byte aligned")
    _refused(call(filter=_filter(n_filters=0)), "n_filters")
    for kw in (dict(nq=-1), dict(n_docs=0), dict(k=0), dict(k=1025)):
        _refused(call(**kw), "need n_docs > 0")
    for d in (0, 32, 96, 1088):
        _refused(call(dim_pad=d), "multiple of 64")
    _refused(call(doc_base=-1), "doc_base")
    _refused(call(doc_base=2 ** 31 - 1 - 1000), "doc_base")
    for null in ("corpus", "queries", "out_doc", "out_score", "out_count"):
        _refused(call(**{null: None}), "null pointer")
    _refused(call(corpus=P[0] + 4), "16-byte aligned")
    _refused(call(queries=P[2] + 4), "16-byte aligned")
    assert call(ws=None) == -3 and call(ws_bytes=64) == -3  # SRX_ERR_NOMEM
    assert call(filter=_filter(), ws=None) == -3            # a good filter passes its check
    assert b"srx_dense_search_half" in L.srx_last_error()
    assert call(nq=0, queries=None) == 0  # nothing to do: no launch


@pytest.mark.parametrize("type_", [0, 1])
def test_score_docs_refusals(type_):
    L = _capi.lib()
    ok = dict(device=0, type=type_, corpus=P[0], n_docs=1000, dim_pad=64, queries=P[2], nq=2, doc_base=0, cand_doc=P[3], cand_count=None, m=5,
              out=P[4], stream=None)
    call = lambda **kw: L.srx_dense_score_docs_half(*{**ok, **kw}.values())
    for t in (-1, 2):
        _refused(call(type=t), "type must be")
    for d in (0, 32, 1088):
        _refused(call(dim_pad=d), "multiple of 64")
    _refused(call(nq=-1), "nq < 0")
    _refused(call(m=0), "m must be >= 1")
    _refused(call(nq=2 ** 20, m=2 ** 12), "nq * m")
    for n in (0, -1, 2 ** 31 - 1):
        _refused(call(n_docs=n), "n_docs")
    _refused(call(doc_base=-1), "doc_base")
    for null in ("corpus", "queries", "cand_doc", "out"):
        _refused(call(**{null: None}), "null pointer")
    _refused(call(corpus=P[0] + 8), "16-byte aligned")
    _refused(call(queries=P[2] + 8), "16-byte aligned")
    assert b"srx_dense_score_docs_half" in L.srx_last_error()
    assert call(nq=0, queries=None, cand_doc=None, out=None) == 0  # nothing to do: no launch


# ---- the two roundings ---------------------------------------------------------------------------------------------------------
def _rounding_cases():
    rng = np.random.default_rng(5)
    f = np.float32
    rnd = np.concatenate([rng.standard_normal(4000).astype(f), (rng.standard_normal(2000) * 1e-6).astype(f), (rng.standard_normal(2000) * 3e4).astype(f),
                          rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(f)])
    rnd = rnd[np.isfinite(rnd)]
    # ties of both types: a value exactly between two neighbours, with an even and an odd lower neighbour
    bf_ties = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00008000, 0x00018000, 0x7F7F8000, 0x3F807FFF, 0x3F808001], np.uint32).view(f)
    f16_ties = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 + 2.0 ** -25,
                         65504.0, 65519.99, 65520.0, 70000.0, -70000.0, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25], f)
    sub = np.array([1e-39, -1e-39, 1e-45, 6e-8, -6e-8, 5.9e-8, 2.9e-8, 3.1e-8, 0.0, -0.0, 3.3e38, -3.4e38, np.inf, -np.inf], f)
    return np.concatenate([rnd, bf_ties, f16_ties, sub])


def test_bf16_rounding_is_torchs():
    import torch
    x = _rounding_cases()
    exp = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = half_ref.round_bf16(x)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
    assert not half_ref.finite(half_ref.round_bf16(np.array([np.nan, np.inf], np.float32)), "bf16").any()  # a NaN's code is not specified: its row is zeroed
    assert np.array_equal(half_ref.to_f32(got, "bf16").view(np.uint32), exp.astype(np.uint32) << 16)
    # by hand: ties go to the even neighbour; the largest finite f32 rounds to inf
    assert half_ref.round_bf16(np.array([0x3F808000, 0x3F818000, 0x7F7F8000], np.uint32).view(np.float32)).tolist() == [0x3F80, 0x3F82, 0x7F80]


def test_f16_rounding_is_numpys_and_torchs():
    import torch
    x = _rounding_cases()
    got = half_ref.round_f16(x)
    exp = torch.from_numpy(x).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, exp)
    r = lambda v: int(half_ref.round_f16(np.array([v], np.float32))[0])
    assert (r(1.0 + 2.0 ** -11), r(1.0 + 3 * 2.0 ** -11)) == (0x3C00, 0x3C02)  # ties to even
    assert (r(2.0 ** -25), r(3 * 2.0 ** -25), r(2.0 ** -24)) == (0x0000, 0x0002, 0x0001)  # subnormals
    assert (r(65504.0), r(65519.99), r(65520.0), r(-0.0)) == (0x7BFF, 0x7BFF, 0x7C00, 0x8000)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_convert_restatement(dtype):
    e = np.array([[1.0, -0.0, 0.5], [70000.0, 1.0, 1.0], [1.0, np.nan, 2.0], [3.3e38, 0.0, 0.0], [2.0, 3.0, 4.0]], np.float32)
    codes, flag = half_ref.convert(e, dtype, 64)
    assert codes.shape == (5, 64) and flag == 1 and not codes[:, 3:].any()
    assert not codes[2].any() and codes[4].any() and codes[0, 1] == 0x8000
    assert bool(codes[1].any()) == (dtype == "bf16") and bool(codes[3].any()) == (dtype == "bf16")  # 70 000 and 3.3e38 are finite bf16 values
    assert half_ref.convert(e[[0, 4]], dtype, 64)[1] == 0
    assert np.array_equal(half_ref.to_f32(codes[4, :3], dtype), [2.0, 3.0, 4.0])


# ---- the layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim_pad", [(1, 64), (31, 64), (33, 128), (100, 192), (65, 1024)])
def test_layout_round_trip(n, dim_pad):
    rng = np.random.default_rng(n + dim_pad)
    codes = rng.integers(0, 2 ** 16, (n, dim_pad), dtype=np.uint16)
    packed = half_ref.pack(codes)
    assert packed.dtype == np.uint16 and packed.nbytes == half_ref.half_bytes(n, dim_pad)
    assert np.array_equal(half_ref.unpack(packed, n, dim_pad), codes)
    assert np.array_equal(unpack_half_host(packed.view(np.uint8), n, dim_pad), codes)  # the package's host-side unpack
    # the header's byte offset formula, element by element on a sample, and the lane map it states
    for r, c in [(0, 0), (n - 1, dim_pad - 1), (n // 2, 7), (n // 2, 8), (n - 1, 15), (n - 1, 16), (0, dim_pad - 9)]:
        off = half_ref.byte_offset(r, c, dim_pad)
        assert off % 2 == 0 and packed[off // 2] == codes[r, c], (r, c)
        piece, lane = off // 16, (off // 16) % 64
        assert lane & 31 == r & 31 and (lane >> 5) == (c >> 3) & 1 and piece // 64 == (r >> 5) * (dim_pad // 16) + (c >> 4)
    rows = ((n + 31) // 32) * 32
    pad = half_ref.unpack(packed, rows, dim_pad)[n:]
    assert not pad.any()  # rows past n in the last tile are zeros


def test_exact_scores_and_tol_by_hand():
    q = half_ref.round_codes(np.array([[1.0, -2.0, 3.0, 0.0]], np.float32), "bf16")
    d = half_ref.round_codes(np.array([[2.0, 1.0, -1.0, 5.0], [0.0, 0.0, 0.0, 0.0]], np.float32), "bf16")
    assert half_ref.exact_scores(q, d, "bf16").tolist() == [[-3.0, 0.0]]
    assert half_ref.abs_scores(q, d, "bf16").tolist() == [[7.0, 0.0]]
    assert half_ref.tol(q, d, "bf16").tolist() == [[4 * 2.0 ** -22 * 7.0, 0.0]]


# ---- the Python layer's checks that need no GPU ---------------------------------------------------------------------------------
def test_storage_keyword_and_dtype():
    svc = sparse_rx.RetrievalService(device="cuda:0")
    for bad in ("x", "int8", "fp16", ""):
        with pytest.raises(ValueError, match="storage must be"):
            svc.set_embeddings(np.zeros((4, 8), np.float32), storage=bad)
    assert check_half_dtype("F16") == "f16" and check_half_dtype("bf16") == "bf16"
    for bad in ("f32", "half", None):
        with pytest.raises(ValueError, match="dtype must be"):
            check_half_dtype(bad)
    with pytest.raises(ValueError, match="dtype must be"):
        DenseHalfIndex(np.zeros((4, 8), np.float32), dtype="f64")
    with pytest.raises(ValueError, match="float32"):
        DenseHalfIndex(np.zeros((4, 8), np.float64))
