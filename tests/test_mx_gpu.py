"""The MX dense index on the GPU (include/mx/sparse_rx_mx.h) against tests/mx_ref.py: the stored bytes, exact scores on small
integers, the fp64 bound on Gaussian rows, the search as the ranking of the scorer's bits, filters, the offset, the service."""
import json
import os

import numpy as np
import pytest

import mx_ref as ref
import parity
from test_gpu_parity import _assert_exact

pytestmark = pytest.mark.gpu
DTYPES = list(ref.TYPES)
BASE = 7_000_000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"


def _buffer(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint8)


def _rows(rng, n, dim, dtype):
    """Gaussian rows x a per-block spread of 2^+-6, with the blocks the quantiser has to get right put in: all zero, an f32-subnormal
    amax, an amax of 3.4e38, elements on ties, elements in (max, next power of two) that saturate, elements that round to zero."""
    vals = ref.VALUES[dtype]
    mids, vmax = (vals[:-1] + vals[1:]) / 2, vals[-1]
    nb = ref.pad64(dim) // 32
    e = rng.standard_normal((n, nb, 32)) * np.exp2(rng.integers(-6, 7, (n, nb, 1)))
    pats = [np.zeros(32), rng.standard_normal(32) * 1e-40, np.concatenate([[3.4e38], rng.uniform(-1, 1, 31) * 1e38]),
            8 * np.resize(np.concatenate([[vmax], mids, -mids]), 32), np.resize([vmax * 1.1, -vmax * 1.1, vmax * 1.13, vals[1]], 32) / 8,
            np.resize([vmax, -vals[1] / 4, vals[1] / 4, -vals[1] / 2], 32)]
    for i, p in enumerate(pats):
        e[i % n, (i // n + i) % nb] = p
    return np.ascontiguousarray(e.reshape(n, -1)[:, :dim], dtype=np.float32)


def _expected_buffer(e, dtype):
    codes, scales, flag = ref.quantize(e, dtype)
    return ref.pack(codes, scales, dtype), flag


# ---- 1. conversion: every byte against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [1, 31, 32, 33, 64, 65, 200, 320, 1024])
def test_convert_bytes(dtype, dim):
    import torch
    import sparse_rx
    rng = np.random.default_rng(dim)
    for n in (1, 33, 100):
        e = _rows(rng, n, dim, dtype)
        exp, flag = _expected_buffer(e, dtype)
        ix = sparse_rx.DenseMxIndex(torch.as_tensor(e, device="cuda:0"), dtype=dtype)
        assert flag == 0 and (ix.dim_pad, ix.device_bytes()) == (ref.pad64(dim), exp.size)
        assert np.array_equal(_buffer(ix.corpus), exp), f"{dtype} dim={dim} n={n}"
    codes, scales = ix.corpus_to_host()
    assert np.array_equal(ix.dequantized_to_host(), ref.dequant(*ref.quantize(e, dtype)[:2], dtype)[:, :dim]) and scales.shape == (n, ix.dim_pad // 32)
    assert ix.max_row_norm() == float((ix.dequantized_to_host() ** 2).sum(axis=1).max()) ** 0.5


def _convert_raw(x, dtype, dim_pad, row0, n_total, out, flag):
    import torch
    from sparse_rx import _capi
    from sparse_rx.index import _stream_ptr
    n, dim = x.shape
    _capi.check(_capi.lib().srx_mx_convert(0, ref.TYPES[dtype], x.data_ptr(), x.stride(0), n, dim, dim_pad, row0, n_total, out.data_ptr(),
                                           None if flag is None else flag.data_ptr(), _stream_ptr(torch, out.device)), "srx_mx_convert")


@pytest.mark.parametrize("dtype", DTYPES)
def test_convert_unaligned_chunks_and_non_finite_rows(dtype):
    import torch
    import sparse_rx
    n, dim = 100, 200
    e = _rows(np.random.default_rng(3), n, dim, dtype)
    exp, _ = _expected_buffer(e, dtype)
    wide = torch.zeros((n, dim + 3), dtype=torch.float32, device="cuda:0")
    wide[:, 1: dim + 1] = torch.as_tensor(e, device="cuda:0")
    x = wide[:, 1: dim + 1]  # ld = dim + 3, the base 4 bytes off a 16-byte boundary
    assert x.stride(0) == dim + 3 and x.data_ptr() % 16 == 4
    out = torch.full((exp.size,), 0xAB, dtype=torch.uint8, device="cuda:0")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    _convert_raw(x[32:], dtype, 256, 32, n, out, flag)  # two chunks, the second first
    _convert_raw(x[:32], dtype, 256, 0, n, out, None)
    assert np.array_equal(_buffer(out), exp) and int(flag.item()) == 0
    # a NaN row and an inf row: zeros with scale 127, the flag bit set, the neighbours untouched
    bad = e.copy()
    bad[3, 7], bad[40, 199] = np.nan, -np.inf
    exp_bad, f = _expected_buffer(bad, dtype)
    keep = np.setdiff1d(np.arange(n), [3, 40])
    c0, s0 = ref.unpack(exp, dtype, n, 256)
    c1, s1 = ref.unpack(exp_bad, dtype, n, 256)
    assert f == 1 and np.array_equal(c0[keep], c1[keep]) and np.array_equal(s0[keep], s1[keep]) and not c1[[3, 40]].any() and (s1[[3, 40]] == 127).all()
    _convert_raw(torch.as_tensor(bad, device="cuda:0"), dtype, 256, 0, n, out, flag)
    assert np.array_equal(_buffer(out), exp_bad) and int(flag.item()) == 1
    with pytest.raises(ValueError, match="non-finite"):
        sparse_rx.DenseMxIndex(bad, dtype=dtype)


# ---- 2. exact on representable integers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nq,dim,k", [(33, 1, 64, 1), (257, 5, 200, 10), (300, 33, 320, 300), (130, 129, 1024, 1024), (96, 1025, 64, 3)])
def test_exact_on_small_integers(dtype, n, nq, dim, k):
    """FP8 rows and all queries: integers in [-15, 15]; FP4 rows: +-{0, 1, 2, 3, 4, 6}; every block has its own cap, so the scales
    differ along a row.  One thing the pinned quantiser does to these inputs: a block whose amax is 15 = 1.875 * 2^3 has the scale
    2^-5, 15 * 32 = 480 is above 448 and saturates, so +-15 is stored as +-14 (asserted below: the only change).  The expected
    scores are therefore the integer dot products of the STORED integers; every product and partial sum is an integer < 2^24."""
    import sparse_rx
    rng = np.random.default_rng(n + dim)
    nb = ref.pad64(dim) // 32
    cap = lambda rows: np.repeat(rng.choice([1, 3, 7, 15], (rows, nb)), 32, axis=1)[:, :dim]
    q = np.rint(rng.uniform(-1, 1, (nq, dim)) * cap(nq)).astype(np.float32)
    if dtype == "mxfp8":
        e = np.rint(rng.uniform(-1, 1, (n, dim)) * cap(n)).astype(np.float32)
    else:
        cap4 = np.repeat(rng.choice([1, 2, 4, 6], (n, nb)), 32, axis=1)[:, :dim]
        e = (np.minimum(rng.choice([0, 1, 2, 3, 4, 6], (n, dim)), cap4) * rng.choice([-1, 1], (n, dim))).astype(np.float32)
    qd, dd = ref.operands(q, e, dtype)
    for x, xd, fp8 in ((q, qd, True), (e, dd, dtype == "mxfp8")):
        changed = xd[:, :dim] != x
        assert (np.abs(x[changed]) == 15).all() and (np.abs(xd[:, :dim][changed]) == 14).all() and (fp8 or not changed.any())
    S = (qd @ dd.T).astype(np.float32)
    assert np.abs(qd @ dd.T).max() < 2 ** 24
    ix = sparse_rx.DenseMxIndex(e, dtype=dtype)
    got = ix.score_docs(q, np.tile(np.arange(n, dtype=np.int32), (nq, 1)))
    assert np.array_equal(got.view(np.uint32), S.view(np.uint32)), f"largest |difference| {np.abs(got - S).max()}"
    _assert_exact(ix.search(q, k), parity.dense_topk_rows(S, k), f"{dtype} {(n, nq, dim, k)}")


# ---- 3. Gaussian rows x a per-block spread ---------------------------------------------------------------------------------------
N, NQ = 300, 33


class _Case:
    def __init__(self, dtype, dim):
        import sparse_rx
        rng = np.random.default_rng(dim)
        nb = ref.pad64(dim) // 32
        gauss = lambda n: (rng.standard_normal((n, nb, 32)) * np.exp2(rng.integers(-6, 7, (n, nb, 1)))).reshape(n, -1)[:, :dim].astype(np.float32)
        self.emb, self.q = gauss(N), gauss(NQ)  # Gaussian x a per-block log-uniform spread of 2^+-6: subnormal element codes occur
        self.emb[[31, 32, N - 1]] = self.emb[0]  # one row stored four times
        self.ix = sparse_rx.DenseMxIndex(self.emb, dtype=dtype, doc_base=BASE)
        self.S = self.ix.score_docs(self.q, np.tile(np.arange(N, dtype=np.int32) + BASE, (NQ, 1)))  # the engine's OWN scores of all docs


@pytest.fixture(scope="module")
def cases():
    made = {}
    return lambda dtype, dim: made.setdefault((dtype, dim), _Case(dtype, dim))


def _expected(S, k):
    d, s, c = parity.dense_topk_rows(S, k)
    return np.where(d >= 0, d + BASE, d).astype(np.int32), s, c


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [200, 320])
def test_scores_within_the_bound_and_search_ranks_the_scorers_bits(cases, dtype, dim):
    """Measured on an MI355X: the instruction does NOT accumulate with fp32 precision.  On these rows the largest error is about half
    the bound (2^-17 of the absolute sum where an fp32 chain would lose 2^-22).  With the convert test's directed blocks mixed into the
    rows (ties at 8 x the element values, saturating blocks, f32-subnormal blocks) the error reached 2.1 .. 3.2 x this bound at
    dim 200 / 320 for both types, while the integer cases above stay exact: the loss is inside one instruction, between products of
    very different magnitude."""
    c = cases(dtype, dim)
    qd, dd = ref.operands(c.q, c.emb, dtype)
    err, tol = np.abs(c.S - ref.exact_scores(qd, dd)), ref.tol(qd, dd)
    print(f"{dtype} dim={dim}: largest error / bound {np.max(err / np.maximum(tol, 1e-300)):.3g}")
    assert (err <= tol).all()
    for col in (31, 32, N - 1):  # the row number does not change a doc's bits
        assert np.array_equal(c.S[:, col].view(np.uint32), c.S[:, 0].view(np.uint32))
    for nq in (1, 5, NQ):  # the streaming kernel, and the GEMM ending inside a query tile: neither nq nor k changes them
        for k in (10, N):
            _assert_exact(c.ix.search(c.q[:nq], k), _expected(c.S[:nq], k), f"{dtype} dim={dim} nq={nq} k={k}")


# ---- 4. filter, offset, the scorer's contract -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_and_offset(cases, dtype):
    import sparse_rx
    c = cases(dtype, 200)
    masks = np.stack([np.random.default_rng(9).random(N) < 0.5, np.zeros(N, bool)])
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    q_filter = np.array([(-1, 0, 1)[i % 3] for i in range(NQ)], np.int32)
    s = c.S.copy()
    for i, r in enumerate(q_filter):
        if r >= 0:
            s[i, ~masks[r]] = 0.0
    exp = _expected(s, 100)
    assert (exp[2][q_filter == 1] == 0).all()
    _assert_exact(c.ix.search(c.q, 100, filter=flt, q_filter=q_filter), exp, f"{dtype} filtered, GEMM")
    _assert_exact(c.ix.search(c.q[:3], 100, filter=flt, q_filter=q_filter[:3]), tuple(x[:3] for x in exp), f"{dtype} filtered, stream")
    off = np.float32(np.ceil(np.abs(c.S).max()) + 1.0)  # above max |S|: every doc is rankable
    shifted = c.S + off
    assert shifted.dtype == np.float32 and (shifted > 0).all()
    exp = _expected(shifted, N)
    assert (exp[2] == N).all()
    _assert_exact(c.ix.search(c.q, N, score_offset=float(off)), exp, f"{dtype} offset")


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_docs_contract(cases, dtype):
    c = cases(dtype, 320)
    cand = np.array([[BASE + 5, BASE + 5, -1, BASE - 1, BASE + N, BASE + N - 1, 0] + [BASE + i for i in range(30)],
                     [BASE + 7] * 37], np.int32)  # a duplicate, padding, before and past the corpus; 37 columns: two chunks of 32
    got = c.ix.score_docs(c.q[:2], cand, np.array([37, 4], np.int32))
    want = np.zeros((2, 37), np.float32)
    want[0, [0, 1, 5]] = c.S[0, [5, 5, N - 1]]
    want[0, 7:] = c.S[0, :30]
    want[1, :4] = c.S[1, 7]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 5. the service ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", DTYPES)
def test_service_with_mx_storage(golden_dir, storage):
    import sparse_rx
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    queries = dict(j["queries"])
    live = [q for q in queries if queries[q].strip()]
    dim, n_docs = 96, len(j["corpus"])
    rng = np.random.default_rng(46)
    emb = np.abs(rng.standard_normal((n_docs, dim))).astype(np.float32)
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    svc.set_embeddings(emb, storage=storage)
    assert isinstance(svc._dense, sparse_rx.DenseMxIndex) and svc.get_stats()["embedding_storage"] == storage
    v = np.abs(vecs[live[0]])  # every score > 0: the first pass fills k rows
    S = svc._dense.score_docs(v[None], np.arange(n_docs, dtype=np.int32)[None])
    qd, dd = ref.operands(v[None], emb, storage)
    assert (np.abs(S - ref.exact_scores(qd, dd)) <= ref.tol(qd, dd)).all()  # the scores of the dequantised rows
    got = svc.search_by_vector(v, k=5)
    d, s, c = parity.dense_topk_rows(S, 5)
    assert c[0] == 5 and [r["doc_id"] for r in got] == [svc.doc_ids[i] for i in d[0]]
    assert np.array_equal(np.array([r["score"] for r in got], np.float32).view(np.uint32), s[0].view(np.uint32))
    # an all-negative query: no score is > 0, the shifted pass runs and its rows are re-scored with the caller's f32 rows
    kk = min(n_docs, 1000)
    allk = svc.search_by_vector(-v, k=kk, min_score=-1e9)
    f32 = np.dot(emb.astype(np.float64), -v.astype(np.float64))
    row_of = {x: i for i, x in enumerate(svc.doc_ids)}
    sc = np.array([r["score"] for r in allk])
    assert len(allk) == kk and (np.diff(sc) <= 0).all() and sc.max() < 0
    assert np.abs(sc - f32[[row_of[r["doc_id"]] for r in allk]]).max() < 1e-4  # fp32 dot products of the f32 rows, not MX scores
    got = svc.search_hybrid(queries, vecs, top_k=10, candidates=20, rescore=True, excluded_docs=svc.doc_ids[::2])
    assert any(got[q] for q in live) and all(not set(got[q]) & set(svc.doc_ids[::2]) for q in live)
    with pytest.raises(ValueError, match="not offered with storage"):
        svc.search_hybrid(queries, vecs, top_k=5, mmr_lambda=0.5)
    with pytest.raises(ValueError, match="not offered with storage"):
        svc.diversify({live[0]: {svc.doc_ids[0]: 1.0}}, top_k=1)
    svc.close()
