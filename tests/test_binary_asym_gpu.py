"""Asymmetric scores over the binary index on the GPU (include/asym/sparse_rx_binary_asym.h).  Integer work throughout: every
comparison is exact equality against the NumPy restatement (tests/binary_asym_ref.py), on either route of the search."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import binary_asym_ref as aref  # noqa: E402
import binary_ref as bref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()


def _eq(got, want, label):
    for g, w, name in zip(got, want, ("doc", "score", "count")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
        assert bad.size == 0, (label, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _index(n, dim, doc_base, seed):
    """a corpus with duplicated rows (ties are cut by doc id), centred on a given array"""
    from sparse_rx import binary as bn
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((max(1, n // 2), dim)).astype(np.float32)[rng.integers(0, max(1, n // 2), size=n)]
    center = (0.1 * rng.standard_normal(dim)).astype(np.float32)
    return bn.DenseBinaryIndex(emb, center=center, device=DEV, doc_base=doc_base), emb, center, rng


# ---- 1. the quantiser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_center", [False, True])
@pytest.mark.parametrize("dim", [1, 100, 128, 200, 1024])
def test_quantiser_bit_for_bit(dim, with_center):
    import torch
    from sparse_rx import binary as bn
    rng = np.random.default_rng(dim)
    center = rng.integers(-3, 4, size=dim).astype(np.float32) if with_center else None
    q = rng.standard_normal((40, dim)).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, size=(40, 1)).astype(np.float32)
    pick = lambda: rng.integers(0, dim)
    q[0, pick()] = np.nan
    q[1, pick()] = np.inf
    q[2, pick()] = -np.inf
    q[3] = 0.0 if center is None else center                              # r all zeros
    q[4] = rng.choice(np.array([1e-45, -3e-45, 0.0, 1e-39], np.float32), size=dim)  # a subnormal maximum (no centre: with one, plain rows)
    q[5] = np.nan
    k = np.resize(np.arange(14, -15, -1), dim).astype(np.float32)         # products exactly k / 2: r = k / 14 * amax, amax = 14 * 2^j
    q[6] = k if center is None else k + center                            # exact next to the integer centre
    q[7], q[8] = k * np.float32(2.0 ** -20), k * np.float32(2.0 ** 40)
    ix = bn.DenseBinaryIndex(np.zeros((1, dim), np.float32), center=center, device=DEV)
    want = aref.quantize(q, center)
    assert want.shape == (40, ix.dim_pad) and np.abs(want[6, :dim]).max() == 7 and (center is not None or set(np.unique(want[4])) <= {-7, 0, 7})
    wide = torch.full((40, dim + 3), 5.0, dtype=torch.float32, device=DEV)  # ld > dim
    wide[:, :dim] = torch.from_numpy(q).to(DEV)
    for x in (torch.from_numpy(q).to(DEV), wide[:, :dim]):
        assert np.array_equal(ix.quantize_queries_device(x).cpu().numpy(), want), (dim, with_center)


# ---- 2. the search, either route ------------------------------------------------------------------------------------------------
CASES = [  # dim, n_docs, nq, m, doc_base, filtered
    (100, 1, 1, 1, 0, False),
    (128, 63, 3, 10, 5, False),
    (200, 65, 33, 1024, 0, True),     # m > n_docs
    (1024, 129, 129, 10, 7, True),    # a second 128-query tile with one query
    (128, 129, 1030, 10, 0, True),    # a second pass, a partial 32-query operand
    (200, 40000, 3, 1024, 0, False),  # two row splits
    (768, 40000, 33, 10, 3, True),
]


def _masks(n, rng):
    masks = np.zeros((3, n), bool)
    masks[0] = rng.random(n) < 0.5
    masks[2, : min(n, 5)] = True  # row 1 allows nothing
    return masks


@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_search_equals_the_restatement(case, route):
    import sparse_rx
    dim, n, nq, m, base, filtered = case
    ix, emb, center, rng = _index(n, dim, base, seed=n + nq)
    qv = rng.standard_normal((nq, dim)).astype(np.float32)
    qv[0] = emb[0]  # the rows equal to doc 0 tie at the top
    masks = _masks(n, rng) if filtered else None
    q_filter = [int(r) for r in np.resize([0, -1, 1, 2], nq)] if filtered else None
    flt = sparse_rx.DocFilter.from_masks(masks, device=DEV, doc_base=base) if filtered else None
    got = ix.asym_search(qv, m, filter=flt, q_filter=q_filter, route=route)
    codes = aref.quantize(qv, center)
    want = aref.search(codes, bref.encode(emb, center), m, base, masks, q_filter)
    _eq(got, want, case)
    if filtered:
        assert want[2][2] == 0 and want[2][3] == min(m, n, 5)  # the row that allows nothing; the row of five docs
    # the scores of given docs: those the search returned, INT32_MIN behind the counts and for -1
    docs = ix.asym_docs(qv, got[0], got[2])
    assert docs.dtype == np.int32 and np.array_equal(docs, got[1]), case
    assert np.array_equal(ix.asym_docs(qv, got[0]), got[1]), case


def test_route_zero_and_given_docs():
    import torch
    from sparse_rx import _capi
    ix, emb, center, rng = _index(300, 200, 11, seed=9)
    d_bits = bref.encode(emb, center)
    for nq in (_capi.SRX_BINARY_ASYM_ROUTE_NQ - 1, _capi.SRX_BINARY_ASYM_ROUTE_NQ):  # either side of the threshold
        qv = rng.standard_normal((nq, 200)).astype(np.float32)
        codes = ix.quantize_queries_device(torch.from_numpy(qv).to(DEV))
        want = aref.search(aref.quantize(qv, center), d_bits, 20, 11)
        for route in (0, 1, 2):
            _eq([t.cpu().numpy() for t in ix.asym_search_device(None, 20, q_codes=codes, route=route)], want, (nq, route))
    cand = rng.integers(0, 330, size=(nq, 70)).astype(np.int32)  # ids below and above the shard, duplicates, padding
    cand[:, 5] = cand[:, 6]
    cand[:, 9] = -1
    count = rng.integers(0, 72, size=nq).astype(np.int32)
    for cc in (None, count):
        assert np.array_equal(ix.asym_docs(qv, cand, cc), aref.score_docs(aref.quantize(qv, center), d_bits, cand, cc, 11))


# ---- 3. the screened search and the service ---------------------------------------------------------------------------------------
def test_screened_asymmetric():
    import sparse_rx
    from sparse_rx import binary as bn
    rng = np.random.default_rng(21)
    n, dim, nq = 700, 96, 5
    centres = rng.standard_normal((8, dim)).astype(np.float32)
    emb = (centres[rng.integers(0, 8, size=n)] + 0.5 * rng.standard_normal((n, dim))).astype(np.float32)
    qv = (centres[:nq] + 0.5 * rng.standard_normal((nq, dim))).astype(np.float32)
    exact = sparse_rx.DenseF32Index(emb, device=DEV)
    binary = bn.DenseBinaryIndex(emb, device=DEV)
    center = binary.center_host()
    masks = np.zeros((2, n), bool)
    masks[0] = rng.random(n) < 0.5
    masks[1, :15] = True
    flt = sparse_rx.DocFilter.from_masks(masks, device=DEV)
    for kw, m_, qf_ in (({}, None, None), ({"filter": flt, "q_filter": [0, 1, -1, 1, 0]}, masks, [0, 1, -1, 1, 0])):
        cover = bn.ScreenedDenseIndex(exact, binary, oversample=4, asymmetric=True)  # 4 * 200 >= 700: the exact search, bit for bit
        _eq(cover.search(qv, 200, **kw), exact.search(qv, 200, **kw), "covering")
        sc = bn.ScreenedDenseIndex(exact, binary, oversample=3, asymmetric=True)
        pd, _, pc = aref.search(aref.quantize(qv, center), bref.encode(emb, center), 30, 0, m_, qf_)
        _eq(sc.search(qv, 10, **kw), bref.cut(pd, exact.score_docs(qv, pd, pc), pc, 10), "pool of 30")
    assert not bn.ScreenedDenseIndex(exact, binary).asymmetric
    with pytest.raises(ValueError, match="asymmetric=True needs a DenseBinaryIndex"):
        bn.ScreenedDenseIndex(exact, sparse_rx.DensePqIndex(emb, dsub=8, device=DEV), asymmetric=True)


def test_service_door(golden_dir):
    import json
    import sparse_rx
    from sparse_rx import binary as bn
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        corpus = json.load(f)["corpus"]
    rng = np.random.default_rng(31)
    n, dim = len(corpus), 64
    emb, vec = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal(dim).astype(np.float32)
    plain, asym, one = (sparse_rx.RetrievalService(device=DEV, tile_log2=6) for _ in range(3))
    for svc, kw in ((plain, {}), (asym, {"screen": "binary_asym", "oversample": n}), (one, {"screen": "binary_asym", "oversample": 1})):
        svc.build_bm25_index(corpus)
        svc.set_embeddings(emb, **kw)
    assert isinstance(asym._dense, bn.ScreenedDenseIndex) and asym._dense.asymmetric and asym.get_stats()["embedding_screen"] == "binary_asym"
    assert plain.search_by_vector(vec, k=7) == asym.search_by_vector(vec, k=7) and len(plain.search_by_vector(vec, k=7)) == 7
    center = one._dense.binary.center_host()
    pool, _, cnt = aref.search(aref.quantize(vec[None, :], center), bref.encode(emb, center), 5)
    assert cnt[0] == 5 and {r["doc_id"] for r in one.search_by_vector(vec, k=5)} <= {one.doc_ids[i] for i in pool[0]}
    for svc in (plain, asym, one):
        svc.close()
    with pytest.raises(ValueError, match="not offered with storage"):
        sparse_rx.RetrievalService(device=DEV).set_embeddings(emb, storage="mxfp8", screen="binary_asym")
