"""The dense family on the GPU at the kernel instances and loop shapes no other test file runs: row lengths between 257 and
512 and the odd trip counts around them (tests/dense_instances.py lists the cases and says which instance each one reaches;
tests/test_dense_instances_cpu.py checks that list against the dispatch lines of the kernel sources).  Nothing is restated
here: the expectations are the NumPy restatements and the helpers of the units' own test files, imported.  Every comparison is
exact -- bytes, integers or fp32 bits -- except the one bound on random half scores, half_ref.tol, which DESIGN.md derives."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import binary_ref  # noqa: E402
import dense_instances as T  # noqa: E402
import half_ref  # noqa: E402
import mmr_ref  # noqa: E402
import quant_ref  # noqa: E402
import rescore_ref  # noqa: E402
import test_binary_gpu as tb  # noqa: E402
import test_half_gpu as th  # noqa: E402
import test_late_gpu as tl  # noqa: E402
import test_mmr_gpu as tm  # noqa: E402
import test_quant_gpu as tqu  # noqa: E402
import test_rescore_gpu as tr  # noqa: E402
from test_gpu_parity import _assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
BASE = th.BASE
assert BASE == T.BASE


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()


def _every_doc(n, nq, base):
    return np.tile(np.arange(n, dtype=np.int32) + base, (nq, 1))


def _residue_filter(n, n_rows, nq):
    """n_rows disjoint masks (row r allows the docs with d % n_rows == r) and q_filter[i] = i % (n_rows + 1) - 1"""
    masks = np.stack([np.arange(n) % n_rows == r for r in range(n_rows)])
    return masks, (np.arange(nq) % (n_rows + 1) - 1).astype(np.int32)


def _set_tail_bits(flt):
    """Ones in every bit of the filter's rows that is not a doc: the rest of the last doc word and the padding words"""
    n = flt.n_docs
    assert n % 32 != 0 and flt.words > n // 32 + 1
    flt.bits[:, n // 32] |= -(1 << (n % 32))
    flt.bits[:, n // 32 + 1:] = -1


# =================================================================================================== the half index
@pytest.mark.parametrize("dtype", T.HALF_TYPES)
@pytest.mark.parametrize("dim,n", T.HALF_CONVERT_CASES)
def test_half_conversion_bytes(dtype, dim, n):
    import torch
    import sparse_rx
    rng = np.random.default_rng(dim * 1000 + n)
    e = th._special_rows(rng, n, dim, dtype)
    codes, flag = half_ref.convert(e, dtype, T.pad64(dim))
    assert flag == 0
    exp = half_ref.pack(codes)
    x = torch.as_tensor(e, device=DEV)
    assert T.half_convert_instance(dim, int(x.stride(0)), x.data_ptr() % 16 == 0) == T.half_convert_instance(dim)  # the load form the table names
    ix = sparse_rx.DenseHalfIndex(x, dtype=dtype)  # ld == dim, one launch
    assert (ix.n_docs, ix.dim, ix.dim_pad, ix.device_bytes()) == (n, dim, T.pad64(dim), exp.nbytes)
    assert np.array_equal(th._corpus_codes(ix), exp), f"{dtype} dim={dim} n={n}"
    assert np.array_equal(ix.corpus_to_host(), codes[:, :dim])


_INT = {}


def _int_world(dtype, n, nq, dim):
    """(index, queries, the exact integer scores) of one shape: built once, shared by the k cases, read-only"""
    import sparse_rx
    key = (dtype, n, nq, dim)
    if key not in _INT:
        d, q, S = th._int_case(n, nq, dim, seed=n * 7 + nq + dim)
        S.setflags(write=False)
        _INT[key] = (sparse_rx.DenseHalfIndex(d, dtype=dtype, doc_base=BASE), q, S)
    return _INT[key]


@pytest.mark.parametrize("dtype", T.HALF_TYPES)
@pytest.mark.parametrize("n,nq,dim,k", T.HALF_INT_CASES)
def test_half_search_and_scorer_on_small_integers(dtype, n, nq, dim, k):
    ix, q, S = _int_world(dtype, n, nq, dim)
    exp = th._expected(S, k, BASE)
    assert exp[2][0] == 0 and (exp[2][1:] > 0).any()
    _assert_exact(ix.search(q, k), exp, f"{dtype} n={n} nq={nq} dim={dim} k={k} n_stages={T.half_n_stages(dim)}")
    cand = np.ascontiguousarray(_every_doc(n, nq, BASE)[:, ::-1])  # every doc, in reverse order
    got = ix.score_docs(q, cand)
    assert np.array_equal(got.view(np.uint32), (S[:, ::-1] + F(0.0)).view(np.uint32))


@pytest.mark.parametrize("dtype", T.HALF_TYPES)
@pytest.mark.parametrize("n,dim", T.HALF_RANDOM_CASES)
def test_half_random_scores_and_ranking(dtype, n, dim):
    import sparse_rx
    nq = 33
    rng = np.random.default_rng(1000 + n + dim)
    emb = rng.standard_normal((n, dim)).astype(F)
    q = rng.standard_normal((nq, dim)).astype(F)
    ix = sparse_rx.DenseHalfIndex(emb, dtype=dtype, doc_base=BASE)
    S = ix.score_docs(q, _every_doc(n, nq, BASE))
    dim_pad = T.pad64(dim)
    dc, _ = half_ref.convert(emb, dtype, dim_pad)
    qc, _ = half_ref.convert(q, dtype, dim_pad)
    exact, tol = half_ref.exact_scores(qc, dc, dtype), half_ref.tol(qc, dc, dtype)
    err = np.abs(S.astype(np.float64) - exact)
    rel = float((err / half_ref.abs_scores(qc, dc, dtype)).max())
    print(f"half {dtype} {(n, dim)}: max |S - exact| / sum|q d| = {rel:.3e} (bound {dim_pad * 2.0 ** -22:.3e})")
    assert (err <= tol).all(), f"{dtype} {(n, dim)}: {int((err > tol).sum())} scores outside the bound, worst ratio {rel:.3e}"
    assert (S < 0).any() and (S > 0).any() and err.max() > 0
    for k in (10, 100, 1024):  # the GEMM and the gathering scorer agree on every bit
        _assert_exact(ix.search(q, k), th._expected(S, k, BASE), f"{dtype} {(n, dim)} k={k}")


@pytest.mark.parametrize("dtype", T.HALF_TYPES)
@pytest.mark.parametrize("n,dim,nq,k,n_rows", T.HALF_FILTER_CASES)
def test_half_filter_across_query_tiles_and_passes(dtype, n, dim, nq, k, n_rows):
    import sparse_rx
    assert T.half_passes(nq, n)[0] == 2
    d, q, S = th._int_case(n, nq, dim, seed=n + nq)
    masks, q_filter = _residue_filter(n, n_rows, nq)
    exp = th._filtered_expected(S, masks, q_filter, k)
    # what the test can see: a second-pass query ranked under the row of the query 1024 places before it gives another row
    first = T.HALF_PASS
    assert (q_filter[first:] != q_filter[: nq - first]).all()
    wrong = th._filtered_expected(S[first:], masks, q_filter[: nq - first], k)
    for i in range(nq - first):
        assert exp[2][first + i] > 0 and not np.array_equal(exp[0][first + i], wrong[0][i]), i
    ix = sparse_rx.DenseHalfIndex(d, dtype=dtype, doc_base=BASE)
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    _assert_exact(ix.search(q, k, filter=flt, q_filter=q_filter), exp, f"{dtype} filtered, nq={nq}")
    _set_tail_bits(flt)
    _assert_exact(ix.search(q, k, filter=flt, q_filter=q_filter), exp, f"{dtype} filtered, nq={nq}, ones in the tail bits")


# =================================================================================================== MaxSim
@pytest.mark.parametrize("dtype", T.HALF_TYPES)
@pytest.mark.parametrize("dim,tq", T.MAXSIM_CASES)
def test_maxsim_exact_integers(dtype, dim, tq):
    import late_ref
    ix = tl._index(dtype, dim)
    assert ix.n_docs == tl.N_DOCS and ix.dim_pad == T.pad64(dim) and late_ref.shape_ok(tq, ix.dim_pad) and T.maxsim_shape_ok(tq, dim)
    Tk, ptr = tl._int_store(dim)
    nq, m = 3, 40
    Q = tl._queries(nq, tq, dim, 7 * dim + tq)
    q_cnt = np.array([tq, max(tq - 1, 0), min(tq, 5)], np.int32)
    cand = tl._cands(nq, m, dim + tq)
    assert set(tl.SPECIAL_COUNTS) <= set(np.diff(ptr)[cand[0]].tolist())
    label = f"{dtype} dim {dim} tq {tq} NAB {T.maxsim_nab(tq)} gpb {T.maxsim_gpb(dim)}"
    tl._same(ix.score_docs(Q.astype(F), q_cnt, cand), tl._Exact(Tk, ptr, Q, q_cnt).scores(cand, None), f"scores {label}")
    tl._same(ix.score_docs(Q.astype(F), None, cand), tl._Exact(Tk, ptr, Q, None).scores(cand, None), f"scores, NULL token counts, {label}")


@pytest.mark.parametrize("dtype", T.HALF_TYPES)
@pytest.mark.parametrize("dim,tq,m,k", T.MAXSIM_RERANK_CASES)
def test_maxsim_rerank(dtype, dim, tq, m, k):
    nq = 4
    ix = tl._index(dtype, dim)
    Tk, ptr = tl._int_store(dim)
    Q = tl._queries(nq, tq, dim, 51 + m)
    Q[3] = 0  # every doc scores +0 for query 3: the ranking is by ascending doc id
    ex = tl._Exact(Tk, ptr, Q, None)
    cand = tl._cands(nq, m, 52 + m, distinct=True)
    cand[0, 3], cand[1, 9] = -1, tl.N_DOCS  # dead positions are never listed
    counts = np.array([m, m // 2, m, m], np.int32)
    for cc in (None, counts):
        got = ix.rerank(Q.astype(F), None, cand, cc, k)
        for g, e, what in zip(got, ex.ranked(cand, cc, k), ("doc", "score", "count")):
            tl._same(g, e, f"rerank {dtype} dim {dim} tq {tq} m {m} k {k} counts {cc is not None}: {what}")
    d, s, n = got
    assert n.tolist() == [m - 1, m // 2 - 1, m, m] and (np.diff(d[3, : n[3]]) > 0).all() and (tl._bits(s[3]) == 0).all()


# =================================================================================================== MMR
def _mmr_check(storage, dim, m):
    ix, rows = tm._world(storage, dim)
    k = min(10, m)
    rng = np.random.default_rng(m * 7 + dim + k)
    cd, cr = tm._pool(rng, 5, m)
    out = tm._check(ix, rows, cd, cr, tm._counts(m), k, 0.5, "cosine", f"{storage} dim {dim} m {m}")
    assert out[3].tolist() == [min(k, m), 0, 0, min(k, m), min(k, max(1, m // 2))]
    assert out[4][0].any()


def _mmr_exact(storage, dim, m):
    """tm.test_small_integers_are_exact at one more shape: gram_exact and select_naive_f64 use no engine code"""
    ix, rows = tm._world(storage, dim, "integers")
    rng = np.random.default_rng(dim + m)
    cd, cr = tm._pool(rng, 3, m, grid=True)
    for lam in (0.25, 0.5, 0.75):
        doc, rel, mmr, count, sim = tm._run(ix, cd, cr, None, 10, lam, "dot")
        for q in range(3):
            G = mmr_ref.gram_exact(rows[cd[q] - tm.BASE])
            assert np.array_equal(sim[q].astype(np.float64), G), (storage, dim, m, q)
            picked, values = mmr_ref.select_naive_f64(G, cr[q], np.ones(m, bool), 10, *mmr_ref.weights(lam), mmr_ref.DOT)
            assert count[q] == 10 and doc[q].tolist() == cd[q, picked].tolist(), (storage, lam, q)
            assert np.array_equal(mmr[q].astype(np.float64), values) and np.array_equal(rel[q], cr[q, picked])


@pytest.mark.parametrize("dtype", T.HALF_TYPES)
@pytest.mark.parametrize("dim,m", T.MMR_HALF_CASES)
def test_mmr_half_gram_and_selection(dtype, dim, m):
    _mmr_check(dtype, dim, m)


@pytest.mark.parametrize("dtype", T.HALF_TYPES)
@pytest.mark.parametrize("dim,m", T.MMR_HALF_EXACT_CASES)
def test_mmr_half_small_integers_are_exact(dtype, dim, m):
    _mmr_exact(dtype, dim, m)


@pytest.mark.parametrize("dim,m", T.MMR_F32_CASES)
def test_mmr_f32_gram_and_selection(dim, m):
    _mmr_check("f32", dim, m)


@pytest.mark.parametrize("dim,m", T.MMR_F32_EXACT_CASES)
def test_mmr_f32_small_integers_are_exact(dim, m):
    _mmr_exact("f32", dim, m)


# =================================================================================================== the binary index
BINARY_DIMS = sorted({c[0] for c in T.BINARY_SEARCH_CASES})


@pytest.mark.parametrize("dim", BINARY_DIMS)
def test_binary_search_at_every_instance(dim):
    for _, n, m, base in [c for c in T.BINARY_SEARCH_CASES if c[0] == dim]:
        tb._case(n, dim, 3, m, seed=dim + n + m, doc_base=base, label=(dim, n, m, base, "NJ", T.binary_nj(dim)))
    # one filtered call, the masks of tb.test_filtered_search_rows_and_q_filter
    rng = np.random.default_rng(31)
    n = 200  # the last tile holds docs 192 .. 199
    masks = np.zeros((4, n), bool)
    masks[0] = rng.random(n) < 0.5
    masks[2, rng.choice(n, size=5, replace=False)] = True  # fewer than m
    masks[3, 192:] = True                                  # only docs of the last partial tile
    q_filter = [0, -1, 1, 2, 3, -1, 0, 3]
    ix, emb, qv, got = tb._case(n, dim, len(q_filter), 16, seed=32 + dim, doc_base=1000, masks=masks, q_filter=q_filter)
    assert got[2].tolist() == [16, 16, 0, 5, 8, 16, 16, 8] and set(got[0][4, :8] - 1000) == set(range(192, 200))


@pytest.mark.parametrize("dim", BINARY_DIMS)
def test_binary_encoder_at_every_instance(dim):
    import torch
    bn = tb._bn()
    rng = np.random.default_rng(100 + dim)
    n, W = 129, T.pad128(dim) // 32
    assert 2 <= W // 4 <= 8
    for with_center in (False, True):
        center = rng.standard_normal(dim).astype(F) if with_center else None
        x = tb._rows(rng, n, dim, center)
        want = binary_ref.encode(x, center)
        ix = bn.DenseBinaryIndex(torch.from_numpy(x).to(DEV), center=center, device=DEV)
        assert ix.words == W and np.array_equal(ix.bits.cpu().numpy().view(np.uint32), binary_ref.tile(want)), (dim, with_center)
        assert np.array_equal(ix.bits_to_host(), want)
        assert np.array_equal(ix.encode_queries_device(torch.from_numpy(x).to(DEV)).cpu().numpy().view(np.uint32), want), (dim, with_center)


@pytest.mark.parametrize("dim", [c[0] for c in T.BINARY_DOCS_CASES])
def test_binary_hamming_docs_at_every_nj(dim):
    base = 500
    ix, emb, qv, got = tb._case(150, dim, 3, 160, seed=41 + dim, doc_base=base)  # rows of 150 results and 10 padding entries
    d_bits, q_bits = binary_ref.encode(emb), binary_ref.encode(qv)
    assert ix.words == 4 * T.binary_nj(dim)
    assert np.array_equal(ix.hamming_docs(qv, got[0]), got[1])  # its own rows: the search's distances, padding -1
    cand = np.array([[base + 3, base + 3, -1, base - 1, base + 150, base + 149, base, 2 ** 31 - 1, -5, base + 7] * 7] * 3, np.int32)[:, :67]
    for count in (None, np.array([67, 0, 9], np.int32), np.array([100, -3, 64], np.int32)):
        want = binary_ref.dist_docs(q_bits, d_bits, cand, count, base)
        assert np.array_equal(ix.hamming_docs(qv, cand, count), want), (dim, count)
        assert (want[0, :2] == want[0, 0]).all() and want[0, 2] == -1 and want[0, 3] == -1 and want[0, 4] == -1 and want[0, 5] >= 0


@pytest.mark.parametrize("n,dim,nq,m,n_rows", T.BINARY_FILTER_CASES)
def test_binary_filter_across_query_tiles_and_passes(n, dim, nq, m, n_rows):
    import sparse_rx
    bn = tb._bn()
    assert T.binary_passes(nq, n) == (2, 8)
    rng = np.random.default_rng(n + nq)
    emb, qv = tb._pm1(rng, n, dim), tb._pm1(rng, nq, dim)
    masks, q_filter = _residue_filter(n, n_rows, nq)
    zero = [6, nq - 2]  # filtered queries of both passes whose code is all zeros: distance 0 to the zero rows that pad the last tile
    assert (q_filter[zero] >= 0).all() and zero[1] >= T.BINARY_PASS
    qv[zero] = -1.0
    d_bits, q_bits = binary_ref.encode(emb), binary_ref.encode(qv)
    assert not q_bits[zero].any()
    want = binary_ref.search(q_bits, d_bits, m, BASE, masks, q_filter)
    first = T.BINARY_PASS
    assert (q_filter[first:] != q_filter[: nq - first]).all()
    wrong = binary_ref.search(q_bits[first:], d_bits, m, BASE, masks, q_filter[: nq - first])
    for i in range(nq - first):
        assert want[2][first + i] > 0 and not np.array_equal(want[0][first + i], wrong[0][i]), i
    last_tile = set(range(n // 64 * 64, n))
    assert any(last_tile & set((want[0][i] - BASE).tolist()) == {d for d in last_tile if d % n_rows == q_filter[i]} for i in range(nq) if q_filter[i] >= 0)
    ix = bn.DenseBinaryIndex(emb, center=None, device=DEV, doc_base=BASE)
    flt = sparse_rx.DocFilter.from_masks(masks, device=DEV, doc_base=BASE)
    tb._eq(ix.hamming_search(qv, m, filter=flt, q_filter=q_filter), want, ("filtered", nq))
    _set_tail_bits(flt)
    got = ix.hamming_search(qv, m, filter=flt, q_filter=q_filter)
    assert got[0].max() < BASE + n, "a lane past n_docs of the last tile became a candidate"
    tb._eq(got, want, ("filtered, ones in the tail bits", nq))


# =================================================================================================== the scorers of given docs
ENGINES = {"f32": tr._F32, "u8": tr._U8}


@pytest.mark.parametrize("engine,dim,n_docs", T.SCORE_ROWS_CASES)
def test_score_rows_at_every_bucket(engine, dim, n_docs):
    rng = np.random.default_rng(dim + n_docs)
    h = ENGINES[engine](rng, n_docs, dim)
    live = 0
    for m, nq in T.SCORE_SHAPES:
        live += int(np.count_nonzero(tr._check_scores(h, rng, nq, m, (engine, dim, n_docs, T.score_rows_instance(dim)))))
    assert live > 1000  # the comparison is not one of zeros


@pytest.mark.parametrize("dim,n_docs,packed", T.SCORE_I8_CASES)
def test_score_i8_at_every_glog(dim, n_docs, packed):
    rng = np.random.default_rng(dim + n_docs)
    h = tr._I8(rng, n_docs, dim, packed=packed)
    assert h.ix.packed is packed
    live = 0
    for m, nq in T.SCORE_SHAPES:
        live += int(np.count_nonzero(tr._check_scores(h, rng, nq, m, ("i8", dim, n_docs, packed, "glog", T.score_i8_glog(dim)))))
    assert live > 1000


# =================================================================================================== the quantiser
def _flagged(e):
    """Query rows with a NaN, a row of zeros and a constant row: NONFINITE and DEGENERATE in the flag word"""
    x = e.copy()
    x[5, x.shape[1] // 2] = np.nan
    x[7] = 0
    x[9] = 1e-3
    return x


@pytest.mark.parametrize("dim,n", T.QUANT_CASES)
def test_quantiser_bytes_scales_and_flags(dim, n):
    pi, pu = T.quant_pads(dim)
    assert (pi, pu) == (quant_ref.pad_i8(dim), quant_ref.pad_u8(dim)) and -(-pi // 256) == -(-pu // 256) == 2
    rows, qrows, ri, ru, qi, qu = tqu._case(dim, n)
    assert ri[2] == 0 and ru[2] == 0 and qi[2] == 0 and qu[3] == 0
    packed = rescore_ref.pack_i8(ri[0])  # the fragment order, restated
    views = tqu._views(rows)
    assert {name for name, _ in views} == ({"dense", "slice", "wide"} if dim % 4 == 0 else {"dense", "slice"})
    for name, x in views:
        tqu._assert_same(tqu._i8_rows(x, n, pi), ri, ("i8 rows", dim, n, name))
        got = tqu._i8_rows(x, n, pi, packed=1)
        assert np.array_equal(got[0], packed) and quant_ref.same_bits(got[1], ri[1]) and got[2] == 0, ("i8 rows, packed", dim, n, name)
        tqu._assert_same(tqu._u8_rows(x, n, pu), ru, ("u8 rows", dim, n, name))
    for name, x in tqu._views(qrows):
        tqu._assert_same(tqu._i8_queries(x, n, pi), qi, ("i8 queries", dim, n, name))
        tqu._assert_same(tqu._u8_queries(x, n, pu), qu, ("u8 queries", dim, n, name))
    got = tqu._u8_queries(tqu._dev(qrows), n, pu, codes=False)  # only the de-quantised block wanted
    assert got[0] is None and got[1] is None and quant_ref.same_bits(got[2], qu[2]) and got[3] == 0
    # flagged rows: the defined outputs and both flag bits
    x = _flagged(qrows)
    exp = (quant_ref.i8_rows(x, pi), quant_ref.u8_rows(x, pu), quant_ref.i8_queries(x, pi), quant_ref.u8_queries(x, pu))
    assert (exp[0][2], exp[1][2], exp[2][2], exp[3][3]) == (1, 1, 3, 3)
    for name, d in tqu._views(x):
        tqu._assert_same(tqu._i8_rows(d, n, pi), exp[0], ("i8 rows, flagged", dim, n, name))
        tqu._assert_same(tqu._u8_rows(d, n, pu), exp[1], ("u8 rows, flagged", dim, n, name))
        tqu._assert_same(tqu._i8_queries(d, n, pi), exp[2], ("i8 queries, flagged", dim, n, name))
        tqu._assert_same(tqu._u8_queries(d, n, pu), exp[3], ("u8 queries, flagged", dim, n, name))
