"""The binary dense index on the GPU (include/binary/sparse_rx_binary.h) and the screened search built on it.  Everything is
integer work or the exact index's own score bits, so every comparison is exact equality against the NumPy restatement
(tests/binary_ref.py): codes and layout of the encoder, the (distance ascending, doc ascending) top-m at every size at which the
kernels take another path, filters, the distances of given docs, ``ScreenedDenseIndex`` over f32 and f16 rows, and the service."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import binary_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()


def _bn():
    from sparse_rx import binary
    return binary


def _pm1(rng, n, dim):
    """rows of +-1: with center None the code of a row is its sign pattern"""
    return (rng.integers(0, 2, size=(n, dim)).astype(np.float32) * 2 - 1).astype(np.float32)


def _eq(got, want, label):
    for g, w, name in zip(got, want, ("doc", "dist / score", "count")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (label, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- 1. encode ----------------------------------------------------------------------------------------------------------------
def _encode_raw(x, dim, row0, n_total, center, tiled, out, dim_pad=None):
    """One call of srx_binary_encode on device tensors (x may be a strided view: ld = its row stride)."""
    import torch
    from sparse_rx import _capi
    ld = max(dim, int(x.stride(0)))
    rc = _capi.lib().srx_binary_encode(0, x.data_ptr(), ld, int(x.shape[0]), dim, dim_pad or ref.pad128(dim), row0, n_total,
                                       None if center is None else center.data_ptr(), tiled, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _capi.check(rc, "srx_binary_encode")


SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 3.5], np.float32)


def _rows(rng, n, dim, center):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    pick = rng.random((n, dim)) < 0.2
    x[pick] = SPECIAL[rng.integers(0, len(SPECIAL), size=int(pick.sum()))]
    if center is not None:  # x == center exactly, in a tenth of the places
        same = rng.random((n, dim)) < 0.1
        x[same] = np.broadcast_to(center, (n, dim))[same]
    return x


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_encode_codes_layout_and_padding(n):
    import torch
    bn = _bn()
    rng = np.random.default_rng(100 + n)
    for dim in (1, 31, 32, 33, 127, 128, 129, 1024):
        W = ref.pad128(dim) // 32
        for with_center in (False, True):
            center = rng.standard_normal(dim).astype(np.float32) if with_center else None
            x = _rows(rng, n, dim, center)
            want = ref.encode(x, center)
            assert not np.unpackbits(want.view(np.uint8), axis=1, bitorder="little")[:, dim:].any()  # bits at or above dim: zero
            label = (n, dim, with_center)
            # the index: tiled, every word of every tile written (the buffer starts as ones)
            ix = bn.DenseBinaryIndex(torch.from_numpy(x).to(DEV), center=center, device=DEV)
            assert ix.device_bytes() == bn.binary_bytes(n, 32 * W, True) and ix.words == W
            assert np.array_equal(ix.bits_to_host(), want), label
            assert np.array_equal(ix.bits.cpu().numpy().view(np.uint32), ref.tile(want)), label  # padding rows and bits: zeros
            assert np.array_equal(ix.center_host(), np.zeros(dim, np.float32) if center is None else center)
            # ld > dim: a column slice of a wider matrix; the buffer prefilled with ones
            wide = torch.full((n, dim + 3), 7.0, dtype=torch.float32, device=DEV)
            wide[:, :dim] = torch.from_numpy(x).to(DEV)
            cdev = None if center is None else torch.from_numpy(center).to(DEV)
            out = torch.full((bn.binary_bytes(n, 32 * W, True) // 4,), -1, dtype=torch.int32, device=DEV)
            _encode_raw(wide[:, :dim], dim, 0, n, cdev, 1, out)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.tile(want)), label
            # the row-major form (queries): exactly the rows' words, nothing behind them
            q = torch.full((n + 1, W), -1, dtype=torch.int32, device=DEV)
            _encode_raw(wide[:, :dim], dim, 0, n, cdev, 0, q)
            got = q.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:n], want) and (got[n] == 0xFFFFFFFF).all(), label
            assert np.array_equal(ix.encode_queries_device(torch.from_numpy(x).to(DEV)).cpu().numpy().view(np.uint32), want), label


def test_encode_chunks_meet_at_tile_edges():
    import torch
    bn = _bn()
    rng = np.random.default_rng(7)
    n, dim = 333, 200
    center = rng.standard_normal(dim).astype(np.float32)
    x = _rows(rng, n, dim, center)
    want = ref.encode(x, center)
    # a host array streamed in chunks of 64 and of 128 rows; a memory-map-like read-only array
    x.setflags(write=False)
    for rows in (64, 128, 448):
        ix = bn.DenseBinaryIndex.from_embeddings(x, center=center, device=DEV, chunk_rows=rows)
        assert np.array_equal(ix.bits.cpu().numpy().view(np.uint32), ref.tile(want)), rows
    for rows in (0, 32, 96):
        with pytest.raises(ValueError, match="multiple of 64"):
            bn.DenseBinaryIndex.from_embeddings(x, center=center, device=DEV, chunk_rows=rows)
    # raw calls out of order, row-major chunks at any row0
    xd, cdev = torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(center).to(DEV)
    out = torch.full((bn.binary_bytes(n, 256, True) // 4,), -1, dtype=torch.int32, device=DEV)
    for lo, hi in ((192, 333), (0, 64), (64, 192)):
        _encode_raw(xd[lo:hi], dim, lo, n, cdev, 1, out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.tile(want))
    q = torch.full((n, 8), -1, dtype=torch.int32, device=DEV)
    for lo, hi in ((100, 333), (0, 33), (33, 100)):
        _encode_raw(xd[lo:hi], dim, lo, n, cdev, 0, q)
    assert np.array_equal(q.cpu().numpy().view(np.uint32), want)
    # the mean as centre: fixed once, data from then on -- the restatement is GIVEN the array
    y = (rng.standard_normal((n, 64)) + 3.0).astype(np.float32)
    for emb in (y, torch.from_numpy(y).to(DEV)):
        ix = bn.DenseBinaryIndex.from_embeddings(emb, device=DEV, chunk_rows=128)
        c = ix.center_host()
        assert c.dtype == np.float32 and c.shape == (64,) and np.array_equal(c, ix.center.cpu().numpy()) and (np.abs(c - 3.0) < 0.5).all()
        assert np.array_equal(ix.bits_to_host(), ref.encode(y, c))
    with pytest.raises(ValueError, match="not supported by the binary engine"):
        bn.DenseBinaryIndex(np.zeros((2, 1025), np.float32), device=DEV)


# ---- 2. search ----------------------------------------------------------------------------------------------------------------
def _case(n, dim, nq, m, seed, doc_base=0, masks=None, q_filter=None, n_patterns=None, label=None):
    import sparse_rx
    bn = _bn()
    rng = np.random.default_rng(seed)
    if n_patterns:
        pat = _pm1(rng, n_patterns, dim)
        emb, qv = pat[rng.integers(0, n_patterns, size=n)], pat[np.arange(nq) % n_patterns]
    else:
        emb, qv = _pm1(rng, n, dim), _pm1(rng, nq, dim)
    ix = bn.DenseBinaryIndex(emb, center=None, device=DEV, doc_base=doc_base)
    d_bits, q_bits = ref.encode(emb), ref.encode(qv)
    flt = None if masks is None else sparse_rx.DocFilter.from_masks(masks, device=DEV, doc_base=doc_base)
    got = ix.hamming_search(qv.reshape(nq, dim), m, filter=flt, q_filter=q_filter)
    want = ref.search(q_bits, d_bits, m, doc_base, masks, q_filter)
    _eq(got, want, label or (n, dim, nq, m))
    return ix, emb, qv, got


def _sizes():
    bn = _bn()
    s = {1, 63, 64, 65}
    for edge in (bn.BLOCK_DOCS, bn.RANK_CHUNK, bn.SPLIT_DOCS, 2 * bn.SPLIT_DOCS):  # workgroup, rank step, one split, two splits
        s |= {edge - 1, edge, edge + 1}
    return sorted(s)


def test_search_at_every_size_edge():
    for n in _sizes():
        for m in (1, 65):
            _case(n, 32, 3, m, seed=n + m)  # m > n_docs for the small sizes: count = n_docs, the row padded


@pytest.mark.parametrize("n,m,nq", [(1, 1024, 1), (64, 64, 2), (65, 64, 2), (5000, 1024, 2), (65537, 1024, 2), (32769, 64, 33)])
def test_search_m_edges_and_merge_capacity(n, m, nq):
    _case(n, 40, nq, m, seed=n + m + nq)  # (65537, 1024): four splits of 1024 = the 4096 entries one merge level takes


@pytest.mark.parametrize("nq", [0, 1, 33, 129, 1025])
def test_search_query_counts(nq):
    bn = _bn()
    assert (bn.QUERY_TILE + 1, bn.PASS_QUERIES + 1) == (129, 1025)  # one above the query tile, one above the pass
    ix, emb, qv, got = _case(300, 70, nq, 10, seed=nq)
    assert got[0].shape == (nq, 10)


def test_search_massive_ties_across_chunks_and_splits():
    bn = _bn()
    n = 2 * bn.SPLIT_DOCS + bn.RANK_CHUNK + 17  # two splits; every tie class spans every chunk
    assert bn.search_plan(4, n, 1000)[1] == 2
    ix, emb, qv, got = _case(n, 32, 4, 1000, seed=11, n_patterns=4)
    doc, dist, cnt = got
    assert (cnt == 1000).all() and len(np.unique(dist)) <= 4
    for q in range(4):  # the boundary falls inside a class: its members are the smallest doc ids of the class
        last = dist[q, -1]
        cls = np.flatnonzero(ref.distances(ref.encode(qv[q: q + 1]), ref.encode(emb))[0] == last)
        taken = doc[q][dist[q] == last]
        assert len(cls) > len(taken) and np.array_equal(taken, cls[: len(taken)])
    _case(n, 32, 4, 1, seed=12, n_patterns=4)
    _case(bn.RANK_CHUNK + 5, 32, 2, 1024, seed=13, n_patterns=4)


def test_search_dim_1024_complement_and_doc_base():
    bn = _bn()
    rng = np.random.default_rng(21)
    n, dim, base = 200, 1024, 7_000_000
    emb = _pm1(rng, n, dim)
    qv = np.stack([-emb[5], emb[5], _pm1(rng, 1, dim)[0]])
    ix = bn.DenseBinaryIndex(emb, center=None, device=DEV, doc_base=base)
    got = ix.hamming_search(qv, n + 3)
    _eq(got, ref.search(ref.encode(qv), ref.encode(emb), n + 3, base), "dim 1024")
    assert got[1][0, n - 1] == 1024 and got[0][0, n - 1] == base + 5 and got[1][1, 0] == 0 and got[0][1, 0] == base + 5
    assert (got[2] == n).all() and (got[0][:, n:] == -1).all() and (got[1][:, n:] == -1).all()
    # q_bits= : the same rows from codes the caller already holds
    import torch
    qb = ix.encode_queries_device(torch.from_numpy(qv).to(DEV))
    again = ix.hamming_search_device(None, n + 3, q_bits=qb)
    _eq([t.cpu().numpy() for t in again], got, "q_bits=")
    with pytest.raises(ValueError):
        ix.hamming_search_device(torch.from_numpy(qv).to(DEV), 5, q_bits=qb)
    for m in (0, 1025):
        with pytest.raises(ValueError):
            ix.hamming_search(qv, m)


# ---- 3. filters ---------------------------------------------------------------------------------------------------------------
def test_filtered_search_rows_and_q_filter():
    rng = np.random.default_rng(31)
    n = 200  # the last tile holds docs 192 .. 199
    masks = np.zeros((4, n), bool)
    masks[0] = rng.random(n) < 0.5
    masks[2, rng.choice(n, size=5, replace=False)] = True  # fewer than m
    masks[3, 192:] = True                                  # only docs of the last partial tile
    q_filter = [0, -1, 1, 2, 3, -1, 0, 3]
    for base in (0, 1000):
        ix, emb, qv, got = _case(n, 96, len(q_filter), 16, seed=32, doc_base=base, masks=masks, q_filter=q_filter)
        assert got[2].tolist() == [16, 16, 0, 5, 8, 16, 16, 8]
        assert (got[0][2] == -1).all() and set(got[0][4, :8] - base) == set(range(192, 200))
    _case(n, 96, 3, 16, seed=33, masks=masks[0], q_filter=None)  # one row for every query


def test_filtered_search_across_splits():
    bn = _bn()
    n = 2 * bn.SPLIT_DOCS + 100
    rng = np.random.default_rng(34)
    masks = np.zeros((3, n), bool)
    masks[0] = rng.random(n) < 0.3
    masks[1, n - 40:] = True
    masks[2, :: 4096] = True
    _case(n, 32, 5, 100, seed=35, masks=masks, q_filter=[0, 1, 2, -1, 0], n_patterns=6)


# ---- 4. distances of given docs ------------------------------------------------------------------------------------------------
def test_dist_docs_equals_the_search_and_the_restatement():
    import torch
    base = 500
    ix, emb, qv, got = _case(150, 200, 3, 160, seed=41, doc_base=base)  # rows of 150 results and 10 padding entries
    d_bits, q_bits = ref.encode(emb), ref.encode(qv)
    assert np.array_equal(ix.hamming_docs(qv, got[0]), got[1])  # its own rows: the search's distances, padding -1
    cand = np.array([[base + 3, base + 3, -1, base - 1, base + 150, base + 149, base, 2 ** 31 - 1, -5, base + 7] * 7] * 3, np.int32)[:, :67]
    for count in (None, np.array([67, 0, 9], np.int32), np.array([100, -3, 64], np.int32)):
        want = ref.dist_docs(q_bits, d_bits, cand, count, base)
        assert np.array_equal(ix.hamming_docs(qv, cand, count), want), count
        assert (want[0, :2] == want[0, 0]).all() and want[0, 2] == -1 and want[0, 3] == -1 and want[0, 4] == -1 and want[0, 5] >= 0
    qb = ix.encode_queries_device(torch.from_numpy(qv).to(DEV))
    out = ix.hamming_docs_device(None, torch.from_numpy(cand).to(DEV), q_bits=qb)
    assert np.array_equal(out.cpu().numpy(), ref.dist_docs(q_bits, d_bits, cand, None, base))
    assert ix.hamming_docs_device(None, torch.zeros((0, 4), dtype=torch.int32, device=DEV), q_bits=qb[:0]).shape == (0, 4)


# ---- 5. the screened search ----------------------------------------------------------------------------------------------------
def _exact(kind, emb, doc_base=0):
    import sparse_rx
    if kind == "f32":
        return sparse_rx.DenseF32Index(emb, device=DEV, doc_base=doc_base)
    return sparse_rx.DenseHalfIndex(emb, dtype=kind, device=DEV, doc_base=doc_base)


@pytest.fixture(scope="module")
def clustered():
    """A small Gaussian mixture: rows near 16 centres, queries near the same centres."""
    rng = np.random.default_rng(51)
    n, dim, nq = 5000, 96, 6
    centres = rng.standard_normal((16, dim)).astype(np.float32)
    emb = (centres[rng.integers(0, 16, size=n)] + 0.5 * rng.standard_normal((n, dim))).astype(np.float32)
    qv = (centres[np.arange(nq) % 16] + 0.5 * rng.standard_normal((nq, dim))).astype(np.float32)
    return emb, qv


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_screened_equals_the_restatement_fed_with_exact_scores(kind, clustered):
    import sparse_rx
    import torch
    bn = _bn()
    emb, qv = clustered
    n, nq, base = emb.shape[0], qv.shape[0], 300
    exact = _exact(kind, emb, base)
    binary = bn.DenseBinaryIndex(emb, device=DEV, doc_base=base)  # centred on the mean
    center = binary.center_host()
    d_bits, q_bits = ref.encode(emb, center), ref.encode(qv, center)
    assert np.array_equal(binary.bits_to_host(), d_bits)
    masks = np.zeros((2, n), bool)
    masks[0] = np.random.default_rng(52).random(n) < 0.4
    masks[1, :15] = True  # fewer allowed docs than the pool
    flt = sparse_rx.DocFilter.from_masks(masks, device=DEV, doc_base=base)
    q_filter = [0, 1, -1, 0, 1, -1]
    for k, oversample, offset in ((10, 4, 0.0), (7, 3, 0.0), (10, 1, 0.0), (300, 4, 0.0), (10, 4, 1000.0), (7, 3, -5.0)):
        sc = bn.ScreenedDenseIndex(exact, binary, oversample)
        pool = ref.screen_pool(k, oversample, n)
        assert sc.pool(k) == pool
        for m_, qf_ in ((None, None), (masks, q_filter)):
            kw = {} if m_ is None else {"filter": flt, "q_filter": qf_}
            pd, _, pc = ref.search(q_bits, d_bits, pool, base, m_, qf_)
            want = ref.cut(pd, exact.score_docs(qv, pd, pc), pc, k, offset)
            got = sc.search(qv, k, score_offset=offset, **kw)
            _eq(got, want, (kind, k, oversample, offset, m_ is not None))
            # the scores of the returned docs are the exact scorer's bits (+ the offset in fp32)
            dev = sc.search_device(torch.from_numpy(qv).to(DEV), k, offset, **({} if m_ is None else {"filter": flt, "q_filter": torch.tensor(qf_, dtype=torch.int32, device=DEV)}))
            s2 = exact.score_docs_device(torch.from_numpy(qv).to(DEV), dev[0], dev[2])
            s2 = (s2 + torch.tensor(offset, dtype=torch.float32, device=DEV)) if offset != 0.0 else s2
            live = torch.arange(k, device=DEV)[None, :] < dev[2][:, None]
            assert torch.equal(torch.where(live, s2, torch.zeros_like(s2)).view(torch.int32), dev[1].view(torch.int32))
            assert (got[2] <= min(k, pool)).all() and (m_ is None or got[2][1] <= 15)
    assert sc.n_docs == n and sc.dim == 96 and sc.doc_base == base and sc.max_row_norm() == exact.max_row_norm()
    cand = np.arange(base, base + 8, dtype=np.int32)[None, :].repeat(nq, 0)
    assert np.array_equal(sc.score_docs(qv, cand), exact.score_docs(qv, cand))
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="oversample"):
            bn.ScreenedDenseIndex(exact, binary, bad)
    with pytest.raises(ValueError, match="the screen speaks of"):
        bn.ScreenedDenseIndex(exact, bn.DenseBinaryIndex(emb[:100], device=DEV, doc_base=base))
    with pytest.raises(ValueError, match="DenseF32Index or a DenseHalfIndex"):
        bn.ScreenedDenseIndex(sparse_rx.DenseUint8Index.from_embeddings(emb[:64], device=DEV), binary)


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_screened_with_a_covering_pool_is_the_exact_search(kind):
    import sparse_rx
    bn = _bn()
    rng = np.random.default_rng(61)
    n, dim, k = 300, 96, 100
    emb, qv = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((5, dim)).astype(np.float32)
    exact = _exact(kind, emb)
    sc = bn.ScreenedDenseIndex(exact, bn.DenseBinaryIndex(emb, device=DEV), oversample=4)
    assert sc.pool(k) == n
    masks = np.zeros((2, n), bool)
    masks[0] = rng.random(n) < 0.5
    masks[1, 290:] = True
    flt = sparse_rx.DocFilter.from_masks(masks, device=DEV)
    bound = float(np.abs(emb.astype(np.float64) @ qv.astype(np.float64).T).max()) * 1.5
    for offset in (0.0, bound):  # the offset makes the negative scores rankable
        for kw in ({}, {"filter": flt, "q_filter": [0, 1, -1, 1, 0]}):
            want = exact.search(qv, k, score_offset=offset, **kw)
            _eq(sc.search(qv, k, score_offset=offset, **kw), want, (kind, offset, bool(kw)))
            if offset and not kw:
                assert (want[2] == k).all()


# ---- 6. the service ------------------------------------------------------------------------------------------------------------
def test_service_screen_covering_pool_changes_nothing(golden_dir):
    import sparse_rx
    bn = _bn()
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    queries = dict(j["queries"])
    live = [q for q in queries if queries[q].strip()]
    dim, n_docs = 96, len(j["corpus"])
    assert n_docs <= 1024  # oversample = n_docs makes the pool cover the corpus
    rng = np.random.default_rng(71)
    emb = rng.standard_normal((n_docs, dim)).astype(np.float32)
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    plain = sparse_rx.RetrievalService(device=DEV, tile_log2=6)
    screened = sparse_rx.RetrievalService(device=DEV, tile_log2=6)
    one = sparse_rx.RetrievalService(device=DEV, tile_log2=6)
    for svc, kw in ((plain, {}), (screened, {"screen": "binary", "oversample": n_docs}), (one, {"screen": "binary", "oversample": 1})):
        svc.build_bm25_index(j["corpus"])
        svc.set_embeddings(emb, **kw)
    st = screened.get_stats()
    assert isinstance(screened._dense, bn.ScreenedDenseIndex) and isinstance(screened._dense.exact, sparse_rx.DenseF32Index)
    assert (st["embedding_storage"], st["embedding_screen"], st["embedding_oversample"]) == ("f32", "binary", n_docs)
    pst = plain.get_stats()
    assert isinstance(plain._dense, sparse_rx.DenseF32Index) and (pst["embedding_screen"], pst["embedding_oversample"]) == (None, None)
    allowed = [d for i, d in enumerate(plain.doc_ids) if i % 3 != 0]
    word = "w3"  # a term of the golden corpus
    calls = [lambda s: s.search_by_vector(vecs[live[0]], k=5),
             lambda s: s.search_by_vector(vecs[live[1]], k=n_docs, min_score=-1e9),  # the second pass: every doc rankable
             lambda s: s.search_by_vector(vecs[live[0]], k=7, allowed_docs=allowed),
             lambda s: s.search_by_vector(vecs[live[0]], k=7, must_terms=[word]),
             lambda s: s.search_hybrid(queries, vecs, top_k=10, candidates=20),
             lambda s: s.search_hybrid(queries, vecs, top_k=10, candidates=20, allowed_docs=allowed),
             lambda s: s.search_hybrid(queries, vecs, top_k=10, candidates=20, must_terms=[word]),
             lambda s: s.search_hybrid(queries, vecs, top_k=10, candidates=20, allowed_docs=allowed, rescore=True)]
    for i, call in enumerate(calls):
        a, b = call(plain), call(screened)
        assert a == b and len(a) > 0 and (isinstance(a, list) or any(a.values())), i
    # oversample = 1: whatever comes back lies in the Hamming pool of its query
    k = 5
    binary = one._dense.binary
    center = binary.center_host()
    for q in live[:4]:
        got = one.search_by_vector(vecs[q], k=k)
        pool, _, cnt = ref.search(ref.encode(vecs[q][None, :], center), ref.encode(emb, center), k)
        assert cnt[0] == k and {r["doc_id"] for r in got} <= {one.doc_ids[i] for i in pool[0]}
    for svc in (plain, screened, one):
        svc.close()
    with pytest.raises(ValueError, match="screen must be None or 'binary'"):
        sparse_rx.RetrievalService(device=DEV).set_embeddings(emb, screen="bogus")
