"""Asymmetric scores over the binary index without a GPU: the twenty-fifth header and its symbol table, the workspace formula, every
refusal the four entry points add (none reaches a device), and the NumPy restatement on cases worked by hand."""
import ctypes
import os
import re

import numpy as np

import binary_asym_ref as aref
import binary_ref as bref
from sparse_rx import _capi, binary as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(16)]  # aligned addresses, never dereferenced


def test_twenty_fifth_header_and_table():
    assert os.listdir(os.path.join(ROOT, "include", "asym")) == ["sparse_rx_binary_asym.h"]
    body = open(os.path.join(ROOT, "include", "asym", "sparse_rx_binary_asym.h")).read().split("#ifndef SPARSE_RX_BINARY_ASYM_H")[1]
    assert set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", body)) == set(_capi.BINARY_ASYM_SYMBOLS) and len(_capi.BINARY_ASYM_SYMBOLS) == 4
    assert not set(_capi.BINARY_ASYM_SYMBOLS) & set(_capi.BINARY_SYMBOLS)
    assert "dense_binary_asym.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "asym", "sparse_rx_binary_asym.h") in _capi._deps()
    assert "include/asym/sparse_rx_binary_asym.h" in _capi.__doc__ and "dense_binary_asym.hip" not in _capi.UNIT_FLAGS
    L = _capi.lib()
    for name, (res, args) in _capi.BINARY_ASYM_SYMBOLS.items():
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == args, name
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", body).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl).split(",")) == len(args), name
    assert re.search(rf"#define SRX_BINARY_ASYM_ROUTE_NQ {_capi.SRX_BINARY_ASYM_ROUTE_NQ}\b", body)
    src = open(os.path.join(_capi.CSRC_DIR, "dense_binary_asym.hip")).read()
    for name, value in (("BA_TILE", bn.TILE_ROWS), ("BA_QTILE", bn.QUERY_TILE), ("BA_PASS", bn.PASS_QUERIES), ("BA_NPT", bn.RANK_CHUNK // 256)):
        assert re.search(rf"constexpr int {name} = {value};", src), name


def test_workspace_formula():
    L = _capi.lib()
    r256 = lambda x: -(-x // 256) * 256
    for nq in (0, 1, 7, 8, 33, 129, 1024, 1030):
        for n in (1, 65, 16384, 40000, 10 ** 6, 2 ** 22 + 1, 2 ** 31 - 2):
            for m in (1, 10, 1024):
                for dim_pad in (128, 768, 1024):
                    QB, ns, base = bn.search_plan(nq, n, m)
                    q32 = -(-min(nq, QB) // 32) * 32
                    want = base + r256(q32 * dim_pad) + r256(4 * q32)
                    assert L.srx_binary_asym_workspace_bytes(nq, n, m, dim_pad) == want, (nq, n, m, dim_pad)
                    assert bn.asym_search_plan(nq, n, m, dim_pad) == (QB, ns, want)
    for nq, n, m, d in ((-1, 10, 1, 128), (1, 0, 1, 128), (1, 10, 0, 128), (1, 10, 1025, 128), (1, 10, 1, 64), (1, 10, 1, 1152), (1, 10, 1, 200)):
        assert L.srx_binary_asym_workspace_bytes(nq, n, m, d) == -1 and L.srx_last_error().startswith(b"srx_binary_asym_workspace_bytes")


def _quant(L, device=0, q=P[0], ld=100, nq=3, dim=100, dim_pad=128, center=P[1], out=P[2], stream=None):
    return L.srx_binary_asym_quantize(device, q, ld, nq, dim, dim_pad, center, out, stream)


def _search(L, device=0, bits=P[0], n_docs=1000, dim_pad=128, q_codes=P[1], nq=3, m=10, doc_base=0, filter=None, out_doc=P[2], out_score=P[3],
            out_count=P[4], workspace=P[5], workspace_bytes=1 << 30, stream=None, route=0):
    return L.srx_binary_asym_search(device, bits, n_docs, dim_pad, q_codes, nq, m, doc_base, filter, out_doc, out_score, out_count, workspace,
                                    workspace_bytes, stream, route)


def _docs(L, device=0, bits=P[0], n_docs=1000, dim_pad=128, q_codes=P[1], nq=3, doc_base=0, cand_doc=P[2], cand_count=P[3], m=10, out=P[4],
          stream=None):
    return L.srx_binary_asym_score_docs(device, bits, n_docs, dim_pad, q_codes, nq, doc_base, cand_doc, cand_count, m, out, stream)


def test_every_refusal_fires_before_a_device_is_touched():
    L = _capi.lib()

    def no(rc, who, word, code=-1):
        msg = L.srx_last_error()
        assert rc == code and word.encode() in msg and msg.startswith(who.encode()), (rc, msg, word)

    who = "srx_binary_asym_quantize"
    no(_quant(L, nq=-1), who, "nq < 0")
    for d in (0, 64, 192, 1152):
        no(_quant(L, dim_pad=d), who, "dim_pad must be a multiple of 128")
    for kw in ({"dim": 0}, {"dim": 129}, {"ld": 99}):
        no(_quant(L, **kw), who, "1 <= dim <= dim_pad and ld >= dim")
    for name in ("q", "out"):
        no(_quant(L, **{name: None}), who, "null pointer")
    no(_quant(L, q=P[0] + 2), who, "4-byte aligned")
    no(_quant(L, center=P[1] + 1), who, "4-byte aligned")
    for off in (1, 4, 8):
        no(_quant(L, out=P[2] + off), who, "out_codes must be 16-byte aligned")
    assert _quant(L, nq=0, q=None, out=None, center=None) == 0

    who = "srx_binary_asym_search"
    for r in (-1, 3, 7):
        no(_search(L, route=r), who, "route must be 0, 1 or 2")
    bad = ctypes.byref(_capi.DocFilterDesc(bits=None, n_filters=2, q_filter=P[7]))
    no(_search(L, filter=bad), who, "null filter bits")
    for kw in ({"nq": -1}, {"n_docs": 0}, {"m": 0}, {"m": 1025}):
        no(_search(L, **kw), who, "need n_docs > 0, 1 <= m <= 1024")
    for d in (0, 64, 192, 1152):
        no(_search(L, dim_pad=d), who, "dim_pad must be a multiple of 128")
    no(_search(L, doc_base=-1), who, "doc_base + n_docs must fit int32")
    no(_search(L, doc_base=2 ** 31 - 1 - 1000), who, "doc_base + n_docs must fit int32")
    for name in ("bits", "q_codes", "out_doc", "out_score", "out_count"):
        no(_search(L, **{name: None}), who, "null pointer")
    no(_search(L, bits=P[0] + 8), who, "16-byte aligned")
    for off in (1, 4, 8):
        no(_search(L, q_codes=P[1] + off), who, "16-byte aligned")
    for route in (0, 1, 2):
        no(_search(L, workspace=None, route=route), who, "workspace too small", code=-3)
        no(_search(L, workspace_bytes=L.srx_binary_asym_workspace_bytes(3, 1000, 10, 128) - 1, route=route), who, "workspace too small", code=-3)
    assert _search(L, nq=0, bits=None, q_codes=None, out_doc=None, out_score=None, out_count=None, workspace=None, workspace_bytes=0) == 0

    who = "srx_binary_asym_score_docs"
    for d in (0, 64, 1152):
        no(_docs(L, dim_pad=d), who, "dim_pad must be a multiple of 128")
    no(_docs(L, nq=-1), who, "nq < 0")
    no(_docs(L, m=0), who, "m must be >= 1")
    no(_docs(L, nq=2 ** 20, m=2 ** 11), who, "nq * m must fit int32")
    for n in (0, 2 ** 31 - 1):
        no(_docs(L, n_docs=n), who, "n_docs out of range")
    no(_docs(L, doc_base=-1), who, "doc_base < 0")
    for name in ("bits", "q_codes", "cand_doc", "out"):
        no(_docs(L, **{name: None}), who, "null pointer")
    no(_docs(L, q_codes=P[1] + 4), who, "16-byte aligned")
    assert _docs(L, nq=0, bits=None, q_codes=None, cand_doc=None, cand_count=None, out=None) == 0


def test_restatement_by_hand():
    for dim_pad in (128, 1024):  # a row of all ones against codes of all +7 / all -7: both ends of the u16 mapping
        ones = bref.encode(np.ones((1, dim_pad), np.float32))
        codes = np.stack([np.full(dim_pad, 7, np.int8), np.full(dim_pad, -7, np.int8)])
        s = aref.scores(codes, ones)
        assert s.tolist() == [[7 * dim_pad], [-7 * dim_pad]]
        assert (s + 7 * dim_pad + 1).tolist() == [[14 * dim_pad + 1], [1]] and 14 * 1024 + 1 < 0xFFFF
    d = bref.encode(np.array([[1, 1, -1], [-1, -1, -1], [1, 1, -1], [1, -1, 1]], np.float32))
    zero = aref.quantize(np.zeros((1, 3), np.float32))
    assert not zero.any() and zero.shape == (1, 128)
    doc, score, cnt = aref.search(zero, d, 5, doc_base=10)  # the all-zero query: every score 0, docs ascending
    assert doc.tolist() == [[10, 11, 12, 13, -1]] and score.tolist() == [[0, 0, 0, 0, aref.INT32_MIN]] and cnt.tolist() == [4]
    q = np.array([[2.0, -1.0, 0.5]], np.float32)  # inv = 3.5: products 7, -3.5 (to even: -4), 1.75 (2)
    codes = aref.quantize(q)
    assert codes[0, :3].tolist() == [7, -4, 2] and not codes[0, 3:].any()
    assert aref.scores(codes, d).tolist() == [[1, -5, 1, 13]]  # e.g. doc 0: 7 - 4 - 2
    doc, score, cnt = aref.search(codes, d, 3, masks=np.array([[1, 1, 1, 0]], bool))
    assert doc.tolist() == [[0, 2, 1]] and score.tolist() == [[1, 1, -5]] and cnt.tolist() == [3]  # the tie: docs ascending
    assert aref.score_docs(codes, d, np.array([[13, 10, 13, -1, 14, 9]]), np.array([5]), doc_base=10).tolist() == [[13, 1, 13, aref.INT32_MIN] + [aref.INT32_MIN] * 2]
    # specials: NaN and inf columns, an infinite and a subnormal maximum
    sp = aref.quantize(np.array([[np.nan, 1.0, -2.0], [np.inf, 1.0, np.nan], [1e-45, 0.0, -1e-45]], np.float32))
    assert sp[:, :3].tolist() == [[0, 4, -7], [0, 0, 0], [7, 0, -7]]
    assert aref.quantize(np.array([[3.0, 5.0]], np.float32), np.array([1.0, 5.0], np.float32))[0, :2].tolist() == [7, 0]
