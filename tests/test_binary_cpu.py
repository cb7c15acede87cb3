"""The binary dense index without a GPU: the seventeenth header and its symbol table, the byte and workspace formulas, every
refusal of the five entry points (none reaches a device), the NumPy restatement on cases worked by hand, and the pool /
sub-list arithmetic of ``ScreenedDenseIndex`` on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import binary_ref as ref
import sparse_rx
from sparse_rx import _capi, binary as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(16)]  # aligned addresses, never dereferenced

OTHER_TABLES = {"SYMBOLS": 35, "RESCORE_SYMBOLS": 4, "QUANT_SYMBOLS": 4, "FILTER_SYMBOLS": 8, "HALF_SYMBOLS": 5, "MMR_SYMBOLS": 3, "TERMS_SYMBOLS": 2,
                "MAXSIM_SYMBOLS": 3, "FIELDS_SYMBOLS": 1, "COLLAPSE_SYMBOLS": 1, "FACET_SYMBOLS": 2, "FEEDBACK_SYMBOLS": 2, "ORDER_SYMBOLS": 3,
                "BOOST_SYMBOLS": 1, "LTR_SYMBOLS": 2, "EVAL_SYMBOLS": 2}
NAMES = {"srx_binary_bytes", "srx_binary_encode", "srx_binary_workspace_bytes", "srx_binary_search", "srx_binary_dist_docs"}


def test_seventeenth_header_and_table():
    assert os.listdir(os.path.join(ROOT, "include", "binary")) == ["sparse_rx_binary.h"]
    hdr = open(os.path.join(ROOT, "include", "binary", "sparse_rx_binary.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef SPARSE_RX_BINARY_H")[1]))
    assert declared == set(_capi.BINARY_SYMBOLS) == NAMES  # five: the column means are taken with torch, there is no sixth call
    assert len(OTHER_TABLES) == 16
    for name, size in OTHER_TABLES.items():
        table = getattr(_capi, name)
        assert len(table) == size, name
        assert not set(_capi.BINARY_SYMBOLS) & set(table)
    assert sum(OTHER_TABLES.values()) + len(_capi.BINARY_SYMBOLS) == 83
    assert "dense_binary.hip" in _capi.SOURCES and os.path.join(_capi.CSRC_DIR, "dense_binary.hip") in _capi._deps()
    assert os.path.join(_capi.INCLUDE_DIR, "binary", "sparse_rx_binary.h") in _capi._deps()
    assert "include/binary/sparse_rx_binary.h" in _capi.__doc__
    L = _capi.lib()
    for name, (res, args) in _capi.BINARY_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    # the argument counts of the declarations
    body = hdr.split("#ifndef SPARSE_RX_BINARY_H")[1]
    for name, (_, args) in _capi.BINARY_SYMBOLS.items():
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", body).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl).split(",")) == len(args), name
    assert {"binary", "DenseBinaryIndex", "ScreenedDenseIndex"} <= set(sparse_rx.__all__)
    assert sparse_rx.DenseBinaryIndex is bn.DenseBinaryIndex and sparse_rx.ScreenedDenseIndex is bn.ScreenedDenseIndex
    # the geometry the module exports is the kernel file's
    src = open(os.path.join(_capi.CSRC_DIR, "dense_binary.hip")).read()
    for name, value in (("BN_TILE", bn.TILE_ROWS), ("BN_QTILE", bn.QUERY_TILE), ("BN_PASS", bn.PASS_QUERIES), ("BN_NPT", bn.RANK_CHUNK // 256)):
        assert re.search(rf"constexpr int {name} = {value};", src), name
    assert bn.SPLIT_DOCS == 4 * bn.RANK_CHUNK and bn.BLOCK_DOCS == 4 * bn.TILE_ROWS and (bn.TILE_ROWS, bn.QUERY_TILE, bn.PASS_QUERIES) == (64, 128, 1024)


def test_byte_and_workspace_formulas():
    L = _capi.lib()
    for n in (0, 1, 63, 64, 65, 1000, 10 ** 7, 2 ** 31 - 2):
        for dim_pad in range(128, 1025, 128):
            W = dim_pad // 32
            assert L.srx_binary_bytes(n, dim_pad, 1) == -(-n // 64) * 64 * W * 4 == bn.binary_bytes(n, dim_pad, True)
            assert L.srx_binary_bytes(n, dim_pad, 0) == n * W * 4 == bn.binary_bytes(n, dim_pad, False)
    for n, dim_pad, tiled in ((-1, 128, 1), (1, 0, 1), (1, 64, 1), (1, 192, 0), (1, 1152, 1), (1, 128, 2), (1, 128, -1)):
        assert L.srx_binary_bytes(n, dim_pad, tiled) == -1 and L.srx_last_error().startswith(b"srx_binary_bytes")
    r256 = lambda x: -(-x // 256) * 256
    for nq in (0, 1, 4, 33, 128, 129, 1024, 1025, 5000):
        for n in (1, 63, 64, 65, 16383, 16384, 32767, 32768, 32769, 10 ** 6, 2 ** 21 + 1, 2 ** 22 + 1, 10 ** 8, 2 ** 31 - 2):
            for m in (1, 10, 64, 65, 1000, 1024):
                ld = -(-n // 64) * 64
                QB = min(max((2 ** 32 // (2 * ld)) // 32 * 32, 32), 1024)
                qb = min(nq, QB)
                ns = max(1, min(2048 // max(qb, 1), n // 16384, 4096 // m))
                want = r256(2 * qb * ld) + 2 * r256(4 * qb * ns * m) + r256(4 * qb * ns) + r256(4 * qb * m) + 256
                assert L.srx_binary_workspace_bytes(nq, n, m) == want, (nq, n, m)
                assert bn.search_plan(nq, n, m) == (QB, ns, want)
    for nq, n, m in ((-1, 10, 1), (1, 0, 1), (1, -1, 1), (1, 10, 0), (1, 10, 1025)):
        assert L.srx_binary_workspace_bytes(nq, n, m) == -1 and L.srx_last_error().startswith(b"srx_binary_workspace_bytes")


def _encode(L, device=0, x=P[0], ld=40, n_rows=100, dim=40, dim_pad=128, row0=0, n_total=100, center=P[1], tiled=1, out=P[2], stream=None):
    return L.srx_binary_encode(device, x, ld, n_rows, dim, dim_pad, row0, n_total, center, tiled, out, stream)


def _search(L, device=0, bits=P[0], n_docs=1000, dim_pad=128, q_bits=P[1], nq=3, m=10, doc_base=0, filter=None, out_doc=P[2], out_dist=P[3],
            out_count=P[4], workspace=P[5], workspace_bytes=1 << 30, stream=None):
    return L.srx_binary_search(device, bits, n_docs, dim_pad, q_bits, nq, m, doc_base, filter, out_doc, out_dist, out_count, workspace,
                               workspace_bytes, stream)


def _docs(L, device=0, bits=P[0], n_docs=1000, dim_pad=128, q_bits=P[1], nq=3, doc_base=0, cand_doc=P[2], cand_count=P[3], m=10, out=P[4],
          stream=None):
    return L.srx_binary_dist_docs(device, bits, n_docs, dim_pad, q_bits, nq, doc_base, cand_doc, cand_count, m, out, stream)


def _filter(bits=P[6], n_filters=2, q_filter=P[7]):
    return ctypes.byref(_capi.DocFilterDesc(bits=bits, n_filters=n_filters, q_filter=q_filter))


def test_every_refusal_fires_before_a_device_is_touched():
    L = _capi.lib()

    def no(rc, who, word, code=-1):
        msg = L.srx_last_error()
        assert rc == code and word.encode() in msg and msg.startswith(who.encode()), (rc, msg, word)

    who = "srx_binary_encode"
    for t in (2, -1):
        no(_encode(L, tiled=t), who, "tiled must be 0 or 1")
    for kw in ({"n_rows": -1}, {"row0": -64}, {"n_total": -1}):
        no(_encode(L, **kw), who, "negative count")
    no(_encode(L, row0=64, n_rows=100), who, "row0 + n_rows > n_total")
    no(_encode(L, row0=128, n_rows=0), who, "row0 + n_rows > n_total")
    for d in (0, 64, 192, 1152, -128):
        no(_encode(L, dim_pad=d), who, "unsupported dim_pad")
    for kw in ({"dim": 0}, {"dim": 129}, {"ld": 39}):
        no(_encode(L, **kw), who, "1 <= dim <= dim_pad and ld >= dim")
    for r in (1, 32, 63):
        no(_encode(L, row0=r, n_rows=10), who, "row0 must be a multiple of 64")
    no(_encode(L, n_rows=2 ** 31 * 64 + 1, n_total=2 ** 31 * 64 + 1), who, "too many rows in one call")
    for name in ("x", "out"):
        no(_encode(L, **{name: None}), who, "null pointer")
    no(_encode(L, x=P[0] + 2), who, "4-byte aligned")
    no(_encode(L, center=P[1] + 1), who, "4-byte aligned")
    for off in (4, 8):
        no(_encode(L, out=P[2] + off), who, "out_bits must be 16-byte aligned")
    # what passes without a launch: no rows (whatever the pointers), and a row-major row0 inside a tile is a matter of tiled
    assert _encode(L, n_rows=0, x=None, out=None, center=None) == 0
    assert _encode(L, n_rows=0, row0=64, tiled=1) == 0 and _encode(L, n_rows=0, row0=33, tiled=0) == 0

    who = "srx_binary_search"
    no(_search(L, filter=_filter(bits=None)), who, "null filter bits")
    no(_search(L, filter=_filter(bits=P[6] + 4)), who, "filter rows must be 16-byte aligned")
    no(_search(L, filter=_filter(n_filters=0)), who, "n_filters must be >= 1")
    for kw in ({"nq": -1}, {"n_docs": 0}, {"n_docs": -5}, {"m": 0}, {"m": 1025}, {"m": -1}):
        no(_search(L, **kw), who, "need n_docs > 0, 1 <= m <= 1024")
    for d in (0, 64, 192, 1152):
        no(_search(L, dim_pad=d), who, "dim_pad must be a multiple of 128")
    no(_search(L, doc_base=-1), who, "doc_base + n_docs must fit int32")
    no(_search(L, doc_base=2 ** 31 - 1 - 1000), who, "doc_base + n_docs must fit int32")
    for name in ("bits", "q_bits", "out_doc", "out_dist", "out_count"):
        no(_search(L, **{name: None}), who, "null pointer")
    no(_search(L, bits=P[0] + 8), who, "16-byte aligned")
    no(_search(L, q_bits=P[1] + 4), who, "16-byte aligned")
    no(_search(L, workspace=None), who, "workspace too small", code=-3)
    no(_search(L, workspace_bytes=L.srx_binary_workspace_bytes(3, 1000, 10) - 1), who, "workspace too small", code=-3)
    no(_search(L, nq=1025, n_docs=40000, workspace_bytes=L.srx_binary_workspace_bytes(1, 40000, 10)), who, "workspace too small", code=-3)
    assert _search(L, nq=0, bits=None, q_bits=None, out_doc=None, out_dist=None, out_count=None, workspace=None, workspace_bytes=0) == 0
    assert _search(L, nq=0, filter=_filter()) == 0

    who = "srx_binary_dist_docs"
    for d in (0, 64, 192, 1152):
        no(_docs(L, dim_pad=d), who, "dim_pad must be a multiple of 128")
    no(_docs(L, nq=-1), who, "nq < 0")
    for m in (0, -1):
        no(_docs(L, m=m), who, "m must be >= 1")
    no(_docs(L, nq=2 ** 20, m=2 ** 11), who, "nq * m must fit int32")
    for n in (0, -1, 2 ** 31 - 1):
        no(_docs(L, n_docs=n), who, "n_docs out of range")
    no(_docs(L, doc_base=-1), who, "doc_base < 0")
    for name in ("bits", "q_bits", "cand_doc", "out"):
        no(_docs(L, **{name: None}), who, "null pointer")
    no(_docs(L, bits=P[0] + 4), who, "16-byte aligned")
    no(_docs(L, q_bits=P[1] + 8), who, "16-byte aligned")
    assert _docs(L, nq=0, bits=None, q_bits=None, cand_doc=None, cand_count=None, out=None) == 0


# ---- the restatement, on cases worked by hand -------------------------------------------------------------------------------
def test_restated_codes_by_hand():
    assert ref.encode(np.array([[1.0]], np.float32)).tolist() == [[1, 0, 0, 0]]                       # dim 1: bit 0 of word 0, dim_pad 128
    assert ref.encode(np.array([[-1.0]], np.float32)).tolist() == [[0, 0, 0, 0]]
    x = np.full((1, 32), 2.0, np.float32)
    assert ref.encode(x).tolist() == [[0xFFFFFFFF, 0, 0, 0]]                                            # dim 32: exactly word 0
    x = np.full((1, 33), 2.0, np.float32)
    assert ref.encode(x).tolist() == [[0xFFFFFFFF, 1, 0, 0]]                                            # dim 33: column 32 is bit 0 of word 1
    x[0, 31] = -2.0
    assert ref.encode(x).tolist() == [[0x7FFFFFFF, 1, 0, 0]]                                            # column 31 is bit 31 of word 0
    # x == center, -0.0, NaN, -inf: 0; +inf: 1; against a centre as well
    special = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, 5.0, 5.0]], np.float32)
    assert ref.encode(special).tolist() == [[0b11101000, 0, 0, 0]]
    center = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 5.0, 4.0], np.float32)
    assert ref.encode(special, center).tolist() == [[0b10101000, 0, 0, 0]]
    assert ref.encode(np.array([[np.inf, np.inf, 1.0]], np.float32), np.array([np.inf, np.nan, np.nan], np.float32)).tolist() == [[0, 0, 0, 0]]
    assert ref.encode(np.zeros((2, 129), np.float32) + 1).shape == (2, 8) and ref.pad128(1024) == 1024 and ref.pad128(1) == 128


def test_restated_distances_and_selection_by_hand():
    rng = np.random.default_rng(5)
    for dim in (1, 32, 33, 1024):
        x = rng.standard_normal((1, dim)).astype(np.float32)
        x[x == 0] = 1.0
        b, c = ref.encode(x), ref.encode(-x)
        assert ref.distances(b, c).tolist() == [[dim]] and ref.distances(b, b).tolist() == [[0]]  # a row and its complement
    d = np.array([[0b0000, 0, 0, 0], [0b0111, 0, 0, 0], [0b0001, 0, 0, 0], [0b1000, 0, 0, 0], [0, 0, 0, 1 << 31]], np.uint32)
    q = np.array([[0, 0, 0, 0]], np.uint32)
    assert ref.distances(q, d).tolist() == [[0, 3, 1, 1, 1]]
    doc, dist, cnt = ref.search(q, d, 3, doc_base=10)
    assert doc.tolist() == [[10, 12, 13]] and dist.tolist() == [[0, 1, 1]] and cnt.tolist() == [3]  # the tie at distance 1: docs ascending
    doc, dist, cnt = ref.search(q, d, 7)
    assert doc.tolist() == [[0, 2, 3, 4, 1, -1, -1]] and dist.tolist() == [[0, 1, 1, 1, 3, -1, -1]] and cnt.tolist() == [5]
    masks = np.array([[0, 1, 0, 1, 1], [0, 0, 0, 0, 0]], bool)
    doc, dist, cnt = ref.search(np.repeat(q, 3, 0), d, 2, masks=masks, q_filter=[0, 1, -1])
    assert doc.tolist() == [[3, 4], [-1, -1], [0, 2]] and dist.tolist() == [[1, 1], [-1, -1], [0, 1]] and cnt.tolist() == [2, 0, 2]
    got = ref.dist_docs(q, d, np.array([[11, 10, 11, -1, 15, 9, 12]]), np.array([6]), doc_base=10)
    assert got.tolist() == [[3, 0, 3, -1, -1, -1, -1]]  # a duplicate, padding, past the shard, before the shard, behind the count


def test_restated_tiling_by_hand():
    for W in (4, 8, 32):
        n4 = W // 4
        want = {(0, 0): 0, (0, 3): 3, (0, 4 % W): (64 * 4 if W > 4 else 0), (0, W - 1): ((n4 - 1) * 64) * 4 + 3,
                (63, 0): 63 * 4, (63, 3): 63 * 4 + 3, (63, W - 1): ((n4 - 1) * 64 + 63) * 4 + 3,
                (64, 0): n4 * 64 * 4, (64, 3): n4 * 64 * 4 + 3, (64, W - 1): ((n4 + n4 - 1) * 64) * 4 + 3}
        if W > 4:
            want[(63, 4)] = (64 + 63) * 4
            want[(64, 4)] = ((n4 + 1) * 64) * 4
        for (r, w), idx in want.items():
            assert ref.tiled_index(r, w, W) == idx == bn.tiled_word_index(r, w, W), (W, r, w)
    rng = np.random.default_rng(6)
    for n, W in ((1, 4), (63, 8), (64, 4), (65, 12), (129, 32)):
        bits = rng.integers(0, 2 ** 32, size=(n, W), dtype=np.uint64).astype(np.uint32)
        buf = ref.tile(bits)
        assert buf.size == -(-n // 64) * 64 * W and buf.size * 4 == bn.binary_bytes(n, 32 * W, True)
        assert np.array_equal(ref.untile(buf, n, W), bits) and np.array_equal(bn.untile_host(buf.view(np.uint8), n, W), bits)
        assert int(np.count_nonzero(buf)) == int(np.count_nonzero(bits))  # padding rows are zeros


def test_restated_cut_by_hand():
    doc = np.array([[7, 3, 9, 5, 1, -1]], np.int32)
    score = np.array([[2.0, 2.0, -1.0, 0.0, 3.0, 9.0]], np.float32)
    d, s, c = ref.cut(doc, score, np.array([5]), 3)
    assert d.tolist() == [[1, 3, 7]] and s.tolist() == [[3.0, 2.0, 2.0]] and c.tolist() == [3]  # > 0 only, ties by doc, behind the count unread
    d, s, c = ref.cut(doc, score, np.array([5]), 6, score_offset=1.5)
    assert d.tolist() == [[1, 3, 7, 5, 9, -1]] and s.tolist() == [[4.5, 3.5, 3.5, 1.5, 0.5, 0.0]] and c.tolist() == [5]
    d, s, c = ref.cut(doc, score, np.array([0]), 2)
    assert d.tolist() == [[-1, -1]] and s.tolist() == [[0.0, 0.0]] and c.tolist() == [0]


# ---- the pool arithmetic of ScreenedDenseIndex -------------------------------------------------------------------------------
def test_pool_and_sublist_arithmetic():
    for k, o, n, want in ((10, 4, 10 ** 6, 40), (10, 1, 10 ** 6, 10), (100, 4, 300, 300), (300, 4, 10 ** 6, 1024), (1024, 1, 2000, 1024),
                          (7, 3, 20, 20), (7, 3, 21, 21), (7, 3, 22, 21), (5, 8, 3, 3)):
        assert bn.screen_pool(k, o, n) == want == ref.screen_pool(k, o, n), (k, o, n)
    assert [bn.pool_lists(p, k) for p, k in ((40, 10), (41, 10), (1024, 300), (3, 5), (21, 7), (1, 1))] == [4, 5, 4, 1, 3, 1]
    counts = bn.sublist_counts(torch.tensor([0, 1, 7, 8, 20, 21], dtype=torch.int32), 3, 7)
    assert counts.dtype == torch.int32 and counts.tolist() == [[0, 0, 0], [1, 0, 0], [7, 0, 0], [7, 1, 0], [7, 7, 6], [7, 7, 7]]
    # k does not divide the pool, and a pool longer than its count: the view pads with -1 / +0.0 behind every count
    rng = np.random.default_rng(7)
    for pool, k, cnt in ((21, 7, [21, 5]), (22, 7, [22, 9]), (10, 4, [3, 10]), (5, 5, [5, 0]), (3, 5, [3, 1]), (1024, 300, [1024, 601])):
        doc = torch.from_numpy(rng.permutation(5000)[: 2 * pool].reshape(2, pool).astype(np.int32))
        score = torch.from_numpy(rng.standard_normal((2, pool)).astype(np.float32))
        count = torch.tensor(cnt, dtype=torch.int32)
        ld, ls, lc = bn.pool_as_lists(doc, score, count, k)
        L = -(-pool // k)
        assert tuple(ld.shape) == tuple(ls.shape) == (2, L, k) and tuple(lc.shape) == (2, L) and ld.is_contiguous() and ls.is_contiguous()
        assert lc.sum(dim=1).tolist() == cnt and int(lc.max()) <= k and int(lc.min()) >= 0
        flat_d, flat_s = ld.reshape(2, L * k), ls.reshape(2, L * k)
        assert torch.equal(flat_d[:, :pool], doc) and torch.equal(flat_s[:, :pool], score)
        assert bool((flat_d[:, pool:] == -1).all()) and bool((flat_s[:, pool:] == 0).all())
        for q in range(2):  # the entries the lists expose are exactly the first count[q] of the pool
            used = [int(ld[q, j, i]) for j in range(L) for i in range(int(lc[q, j]))]
            assert used == doc[q, : cnt[q]].tolist()
    for bad in (0, -1, 1.5, True, "4"):
        with pytest.raises((ValueError, TypeError)):
            bn.check_oversample(bad)
    assert bn.check_oversample(1) == 1 and bn.check_oversample(8) == 8
    for dim, want in ((1, 128), (128, 128), (129, 256), (768, 768), (1024, 1024)):
        assert bn.pad128(dim) == want
    for dim in (0, 1025, 4096):
        with pytest.raises(ValueError):
            bn.pad128(dim)


def test_service_and_pairing_refusals():
    svc = sparse_rx.RetrievalService()
    e = np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError, match="screen must be None or 'binary'"):
        svc.set_embeddings(e, screen="bogus")
    with pytest.raises(ValueError, match="oversample"):
        svc.set_embeddings(e, screen="binary", oversample=0)
    with pytest.raises(ValueError, match="storage"):
        svc.set_embeddings(e, storage="int8", screen="binary")
    assert getattr(svc, "_dense", None) is None
    svc.close()
    with pytest.raises(ValueError, match="DenseF32Index or a DenseHalfIndex"):
        bn.ScreenedDenseIndex(object(), object())
