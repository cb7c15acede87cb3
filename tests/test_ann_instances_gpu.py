"""The PQ, IVF and IVF-PQ indexes on the GPU at the kernel instances and loop shapes their own test files do not run: the scan
instances of 3, 5, 6 and 7 pieces per row, waves that walk several tiles through the double buffer, second passes of every query
loop, probe selections over more than 256 lists, long lists, long member lists, scalar-load assignment, wide candidate blocks
(tests/ann_instances.py lists the cases and says which instance or loop each one reaches; tests/test_ann_instances_cpu.py checks
that list against the dispatch lines of the kernel sources).  Nothing is restated here: the expectations are the NumPy
restatements pq_ref, ivf_ref and ivfpq_ref and the helpers of the units' own test files, imported.  Every comparison is exact:
integers, bytes or fp32 bits.  Where a case needs many or wide rows, the rows are rebuilt from chosen codes (a row that IS its
codewords encodes to them), so that no reference encoder runs over them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ann_instances as T  # noqa: E402
import ivf_ref  # noqa: E402
import ivfpq_ref  # noqa: E402
import pq_ref  # noqa: E402
import test_ivfpq_gpu as tq  # noqa: E402
import test_pq_gpu as tp  # noqa: E402
from test_gpu_parity import _assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
BASE = T.BASE
assert BASE == tp.BASE == tq.BASE and tuple(tq.SIZES) == T.IVFPQ_SIZES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()


def _dev(x):
    import torch
    return torch.as_tensor(x, device=DEV)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _grid_codebooks(rng, M, dsub):
    """f32[M, 256, dsub] on a 2^-10 grid in [-2, 2], no codeword twice in a subspace"""
    cb = (rng.integers(-2048, 2049, (M, 256, dsub)) / 1024.0).astype(F)
    assert all(len(np.unique(cb[m], axis=0)) == 256 for m in range(M))
    return cb


def _filter(n, nq, seed=9):
    """test_bit_for_bit's filter: a random row and an empty row, q_filter of period 3 -> (masks, q_filter, allowed[nq, n])"""
    masks = np.stack([np.random.default_rng(seed).random(n) < 0.5, np.zeros(n, bool)])
    q_filter = np.array([(-1, 0, 1)[j % 3] for j in range(nq)], np.int32)
    return masks, q_filter, np.stack([np.ones(n, bool), masks[0], masks[1]])[q_filter + 1]


def _offset(S):
    return F(np.ceil(np.abs(S).max()) + 1.0)  # above max |S|: every doc is rankable


def _cands(rng, n, m, nq=3):
    """i32[nq, m] and the counts tried: duplicates, padding, docs before and past the corpus, a count shorter than m"""
    cand = (rng.integers(-5, n + 5, (nq, m)) + BASE).astype(np.int32)
    cand[0, :7] = [BASE, BASE, -1, BASE - 1, BASE + n, BASE + n - 1, 0]
    cand[1] = BASE + n // 2
    cand[2, -1] = BASE + n - 1  # the last candidate of the last chunk is a doc
    return cand, (None, np.array([m, 4, m - 700], np.int32), np.array([m + 9, -3, 1024], np.int32))


def _check_scorer(ix, q, S, n, m, label):
    assert T.scorer_grid(m)[1] >= 2
    cand, counts = _cands(np.random.default_rng(m), n, m)
    for count in counts:
        want = pq_ref.score_docs(S, cand, count, BASE)
        if count is None:
            assert np.count_nonzero(want[0]) > m // 2 and want[2, -1] != 0  # the comparison is not one of zeros
        assert np.array_equal(_bits(ix.score_docs(q, cand, count)), _bits(want)), (label, m, None if count is None else count.tolist())


# =================================================================================================== the PQ index
@pytest.mark.parametrize("dsub,dim,n", T.PQ_INSTANCE_CASES)
def test_pq_scan_instances_bit_for_bit(dsub, dim, n):
    assert T.pieces(T.subspaces(dim, dsub)) in (3, 5, 6, 7)
    tp.test_bit_for_bit(dsub, dim, n)  # codes, tables, reconstruction, plain / filtered / offset search, the scorer, a query alone


@pytest.mark.parametrize("dsub,dim,n,nq", T.PQ_DEEP_CASES)
def test_pq_waves_walk_several_tiles(dsub, dim, n, nq):
    import sparse_rx
    M = T.subspaces(dim, dsub)
    walks = T.pq_walks(nq, n, M, _cus())  # with this device's CU count
    assert T.deep(walks) and n % 64 != 0, (M, _cus(), walks)
    rng = np.random.default_rng(dim + n)
    cb = _grid_codebooks(rng, M, dsub)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    x = pq_ref.reconstruct(codes, cb, dim)
    q = (rng.standard_normal((nq, dim)) * np.exp2(rng.integers(-2, 3, (nq, 1)))).astype(F)
    ix = sparse_rx.DensePqIndex(_dev(x), dsub=dsub, codebooks=cb, doc_base=BASE)
    assert np.array_equal(ix.codes_to_host(), codes)
    assert sparse_rx.pq.search_plan(nq, n, M, 10)[:2] == (T.PASS, 1)
    S = pq_ref.scores(pq_ref.lut(q, cb), codes)
    S.setflags(write=False)
    masks, q_filter, allowed = _filter(n, nq)
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    off = _offset(S)
    label = f"dsub={dsub} dim={dim} n={n} nq={nq} walks={sorted(set(walks[0]))}"
    _assert_exact(ix.search(q, 10), pq_ref.search(S, 10, doc_base=BASE), label)
    _assert_exact(ix.search(q, 100, filter=flt, q_filter=q_filter), pq_ref.search(S, 100, allowed=allowed, doc_base=BASE), label + " filtered")
    exp = pq_ref.search(S, 1024, score_offset=off, doc_base=BASE)
    assert (exp[2] == 1024).all() and (exp[0] >= BASE + n // 64 * 64).any()  # docs of the partial last tile rank
    _assert_exact(ix.search(q, 1024, score_offset=float(off)), exp, label + " offset")


@pytest.mark.parametrize("dsub,dim,n,nq", T.PQ_PASS_CASES)
def test_pq_second_pass(dsub, dim, n, nq):
    import sparse_rx
    assert T.pq_passes(nq, n) == [T.PASS, nq - T.PASS]
    x, cb, q = tp._data(np.random.default_rng(nq), n, dim, dsub, nq=nq)
    codes = pq_ref.encode(x, cb)
    ix = sparse_rx.DensePqIndex(_dev(x), dsub=dsub, codebooks=cb, doc_base=BASE)
    assert np.array_equal(ix.codes_to_host(), codes)
    S = pq_ref.scores(pq_ref.lut(q, cb), codes)
    masks, q_filter, allowed = _filter(n, nq)
    first = T.PASS
    assert (q_filter[first:] != q_filter[: nq - first]).all()  # a second-pass query ranked under the row 1024 places before it shows
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    off = _offset(S)
    exp = pq_ref.search(S, 10, doc_base=BASE)
    assert not np.array_equal(exp[0][first:], exp[0][: nq - first])
    _assert_exact(ix.search(q, 10), exp, "two passes")
    _assert_exact(ix.search(q, 10, filter=flt, q_filter=q_filter), pq_ref.search(S, 10, allowed=allowed, doc_base=BASE), "two passes, filtered")
    _assert_exact(ix.search(q, 1024, score_offset=float(off)), pq_ref.search(S, 1024, score_offset=off, doc_base=BASE), "two passes, offset")
    _assert_exact(ix.search(q[first: first + 1], 10), tuple(a[first: first + 1] for a in exp), "query 1024 alone")


_PQ_SCORER = {}


@pytest.mark.parametrize("dsub,dim,n,m", T.PQ_SCORER_CASES)
def test_pq_scorer_chunks(dsub, dim, n, m):
    import sparse_rx
    if (dsub, dim, n) not in _PQ_SCORER:
        x, cb, q = tp._data(np.random.default_rng(dim + n), n, dim, dsub, nq=3)
        codes = pq_ref.encode(x, cb)
        ix = sparse_rx.DensePqIndex(_dev(x), dsub=dsub, codebooks=cb, doc_base=BASE)
        assert np.array_equal(ix.codes_to_host(), codes)
        _PQ_SCORER[dsub, dim, n] = (ix, q, pq_ref.scores(pq_ref.lut(q, cb), codes))
    ix, q, S = _PQ_SCORER[dsub, dim, n]
    _check_scorer(ix, q, S, n, m, "pq")


# =================================================================================================== the IVF index
_PROBE = {}


def _probe_world(nlist, dtype):
    """(index, queries, exact centroid scores): centroids and queries in {-1, 0, 1}, query 0 a unit vector whose scores are the
    crafted column; one doc per centroid.  Built once per nlist, read-only."""
    import sparse_rx
    if (nlist, dtype) not in _PROBE:
        rng = np.random.default_rng(nlist)
        cent = rng.integers(-1, 2, (nlist, T.IVF_DIM)).astype(F)
        cent[:, 0] = T.ivf_crafted_scores(nlist)
        q = rng.integers(-1, 2, (T.PASS + 3, T.IVF_DIM)).astype(F)
        q[0] = 0
        q[0, 0] = 1
        C = ivf_ref.int_scores(q, cent)
        C.setflags(write=False)
        assert (C < 0).any() and (C == 0).any() and np.array_equal(C[0], cent[:, 0])
        _PROBE[nlist, dtype] = (sparse_rx.IvfHalfIndex(_dev(cent.copy()), nlist, dtype=dtype, centroids=cent), q, C)
    return _PROBE[nlist, dtype]


@pytest.mark.parametrize("nlist,nprobe,nq,dtype", T.IVF_PROBE_CASES)
def test_ivf_probe_select_over_many_lists(nlist, nprobe, nq, dtype):
    ix, q, C = _probe_world(nlist, dtype)
    pl, ps = ix.probe(q[:nq], nprobe)
    el, es = ivf_ref.probe(C[:nq], nprobe)
    assert np.array_equal(pl, el) and np.array_equal(_bits(ps), _bits(es)), (nlist, nprobe, nq, dtype)
    # the crafted row: above the threshold everything, at the threshold the lowest-numbered lists only
    value, need, ties, taken = T.ivf_select_ties(T.ivf_crafted_scores(nlist), nprobe)
    at = np.flatnonzero(C[0] == value)
    assert sorted(pl[0][ps[0] == value].tolist()) == at[:need].tolist() and len(at) == sum(ties)
    assert set(np.flatnonzero(C[0] > value).tolist()) <= set(pl[0].tolist())


@pytest.mark.parametrize("nlist,nprobe,nq,dtype", T.IVF_PROBE_PASS_CASES)
def test_ivf_probe_second_pass(nlist, nprobe, nq, dtype):
    ix, q, C = _probe_world(nlist, dtype)
    assert nq == len(q) > T.PASS
    pl, ps = ix.probe(q, nprobe)
    el, es = ivf_ref.probe(C, nprobe)
    assert not np.array_equal(el[T.PASS:], el[: nq - T.PASS])
    assert np.array_equal(pl, el) and np.array_equal(_bits(ps), _bits(es))
    one = ix.probe(q[T.PASS: T.PASS + 1], nprobe)
    assert np.array_equal(one[0], el[T.PASS: T.PASS + 1]) and np.array_equal(_bits(one[1]), _bits(es[T.PASS: T.PASS + 1]))


_SEARCH = {}


def _search_world(dtype):
    """test_ivf_gpu.py's integer construction with one list of 66 tiles: (index, queries, S, C, the list of every doc)"""
    import sparse_rx
    if dtype not in _SEARCH:
        rng = np.random.default_rng(len(dtype))
        nlist = len(T.IVF_SEARCH_SIZES)
        cent = rng.choice([-1.0, 1.0], (nlist, T.IVF_DIM)).astype(F)  # equal norms: a copy of a centroid, scaled, belongs to it
        owner = rng.permutation(np.repeat(np.arange(nlist), T.IVF_SEARCH_SIZES))
        emb = (cent[owner] * rng.choice([1.0, 2.0], (len(owner), 1))).astype(F)
        ix = sparse_rx.IvfHalfIndex(_dev(emb), nlist, dtype=dtype, centroids=cent, doc_base=BASE)
        doc_list = ivf_ref.assign(ivf_ref.int_scores(emb, cent))
        assert np.array_equal(ix.list_sizes(), T.IVF_SEARCH_SIZES) and np.array_equal(doc_list, owner)
        assert ix.max_list_tiles == T.ceil_div(max(T.IVF_SEARCH_SIZES), 32) == 66
        q = rng.integers(-2, 3, (T.PASS + 5, T.IVF_DIM)).astype(F)
        S, C = ivf_ref.int_scores(q, emb), ivf_ref.int_scores(q, cent)
        S.setflags(write=False)
        _SEARCH[dtype] = (ix, q, S, C, doc_list)
    return _SEARCH[dtype]


def _given_lists(nq, nprobe, nlist):
    """A probe_list of the caller: row j starts at list j % nlist; padding and a repeat where the row is long enough"""
    given = ((np.arange(nq)[:, None] + np.arange(nprobe)[None, :] * (1 + np.arange(nq)[:, None] // nlist % 2)) % nlist).astype(np.int32)
    if nprobe >= 3:
        given[::2, 1] = -1
        given[1::2, 2] = given[1::2, 0]
    return given


def _check_ivf_search(dtype, nq, nprobe, k):
    import sparse_rx
    ix, q, S, C, doc_list = _search_world(dtype)
    q, S, C, n = q[:nq], S[:nq], C[:nq], len(doc_list)
    label = f"{dtype} nq={nq} nprobe={nprobe} k={k}"
    assert T.ivf_plan(nq, ix.nlist, nprobe, ix.max_list_tiles)[0] == min(nq, T.PASS)
    el = ivf_ref.probe(C, nprobe)[0]
    exp = ivf_ref.search(S, doc_list, el, k, doc_base=BASE)
    _assert_exact(ix.search(q, k, nprobe), exp, label)
    masks, q_filter, allowed = _filter(n, nq)
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    _assert_exact(ix.search(q, k, nprobe, filter=flt, q_filter=q_filter), ivf_ref.search(S, doc_list, el, k, allowed=allowed, doc_base=BASE), label + " filtered")
    off = _offset(S)
    _assert_exact(ix.search(q, k, nprobe, score_offset=float(off)), ivf_ref.search(S, doc_list, el, k, score_offset=off, doc_base=BASE), label + " offset")
    given = _given_lists(nq, nprobe, ix.nlist)
    want = ivf_ref.search(S, doc_list, given, k, score_offset=off, doc_base=BASE)
    _assert_exact(ix.search(q, k, nprobe, score_offset=float(off), probe_list=given), want, label + " given lists")
    return ix, q, exp, given, want, q_filter, off


@pytest.mark.parametrize("dtype,nq,nprobe,k", T.IVF_SEARCH_CASES)
def test_ivf_search_over_a_long_list(dtype, nq, nprobe, k):
    _check_ivf_search(dtype, nq, nprobe, k)


@pytest.mark.parametrize("dtype,nq,nprobe,k", T.IVF_SEARCH_PASS_CASES)
def test_ivf_search_second_pass(dtype, nq, nprobe, k):
    ix, q, exp, given, want, q_filter, off = _check_ivf_search(dtype, nq, nprobe, k)
    first = T.PASS
    assert T.ivf_passes(nq, T.ivf_plan(nq, ix.nlist, nprobe, ix.max_list_tiles)[0]) == 2
    assert (q_filter[first:] != q_filter[: nq - first]).all() and (given[first:] != given[: nq - first]).any(axis=1).all()
    _assert_exact(ix.search(q[first: first + 1], k, nprobe), tuple(a[first: first + 1] for a in exp), "query 1024 alone")
    _assert_exact(ix.search(q[first: first + 1], k, nprobe, score_offset=float(off), probe_list=given[first: first + 1]),
                  tuple(a[first: first + 1] for a in want), "query 1024 alone, given lists")


@pytest.mark.parametrize("dtype,dim,ld,off", T.IVF_ASSIGN_CASES)
def test_ivf_assign_load_forms(dtype, dim, ld, off):
    import torch
    from sparse_rx import ivf
    nlist, n = T.IVF_ASSIGN_NLIST, T.IVF_ASSIGN_ROWS
    rng = np.random.default_rng(dim * 100 + ld + off)
    cent = rng.choice([-1.0, 1.0], (nlist, dim)).astype(F)
    rows = rng.integers(-2, 3, (n, dim)).astype(F)
    buf = torch.full((n * ld + 8,), 7.0, dtype=torch.float32, device=DEV)  # what lies between the rows would change every score
    assert buf.data_ptr() % 16 == 0
    x = buf[off: off + n * ld].view(n, ld)[:, :dim]
    x.copy_(_dev(rows))
    assert T.ivf_assign_vec(dim, int(x.stride(0)), x.data_ptr() % 16 // 4) == T.ivf_assign_vec(dim, ld, off)  # the load form the table names
    assert x.stride(0) == ld and x.is_contiguous() == (ld == dim)
    packed, _ = ivf.pack_half_device(_dev(cent), dtype)
    lists, best = ivf.assign_device(packed, nlist, dtype, x, with_score=True)
    scores = ivf_ref.int_scores(rows, cent)
    assert np.array_equal(lists.cpu().numpy(), ivf_ref.assign(scores)), (dtype, dim, ld, off)
    assert np.array_equal(_bits(best.cpu().numpy()), _bits(scores.max(axis=1))), (dtype, dim, ld, off)


@pytest.mark.parametrize("dim", [d for (d,) in T.IVF_UPDATE_CASES])
def test_ivf_update_rounds(dim):
    from sparse_rx import ivf
    lens = list(T.IVF_UPDATE_LENS)
    assert max(T.ivf_update_rounds(m)[0] for m in lens) == 3
    rng = np.random.default_rng(90 + dim)
    n = sum(lens) + 17
    rows = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-8, 9, (n, 1)))).astype(F)
    member = np.concatenate([np.sort(m) for m in np.split(rng.permutation(n)[: sum(lens)], np.cumsum(lens)[:-1])]).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    prev = rng.standard_normal((len(lens), dim)).astype(F)
    got = ivf.update_device(_dev(rows), _dev(ptr), _dev(member), _dev(prev)).cpu().numpy()
    exp = ivf_ref.update(rows, ptr, member, prev)
    bad = np.flatnonzero((_bits(got) != _bits(exp)).any(axis=1))
    assert len(bad) == 0, f"dim {dim}: lists of {[lens[c] for c in bad]} members differ"
    assert np.array_equal(got[0], prev[0]) and np.array_equal(got[6], prev[6])


# =================================================================================================== the IVF-PQ index
@pytest.mark.parametrize("dsub,dim,dtype", T.IVFPQ_INSTANCE_CASES)
def test_ivfpq_scan_instances_bit_for_bit(dsub, dim, dtype):
    assert T.pieces(T.subspaces(dim, dsub)) in (3, 5, 7, 8)
    tq.test_bit_for_bit(dsub, dim, dtype)  # codes, reconstruction, probe, plain / filtered / offset / given-list search, the scorer


@pytest.mark.parametrize("dsub,dim,dtype,nq", T.IVFPQ_DEEP_CASES)
def test_ivfpq_waves_walk_across_lists(dsub, dim, dtype, nq):
    import sparse_rx
    sizes, M = T.IVFPQ_DEEP_SIZES, T.subspaces(dim, dsub)
    nlist, n = len(sizes), sum(sizes)
    rng = np.random.default_rng(dim + dsub)
    cent = rng.integers(-4, 5, (nlist, dim)).astype(F)
    lists = rng.permutation(np.repeat(np.arange(nlist), sizes)).astype(np.int32)
    cb = _grid_codebooks(rng, M, dsub)
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    res = pq_ref.reconstruct(codes, cb, dim)
    x = cent[lists] + res  # integers + a 2^-10 grid below 2: exact, and x - centroid is the codeword again
    assert x.dtype == F and np.array_equal(ivfpq_ref.residuals(x, lists, cent, dtype), res)
    q = rng.integers(-3, 4, (nq, dim)).astype(F)
    ix = tq._build(cent, lists, x, cb, dsub, dtype, doc_base=BASE)
    assert np.array_equal(ix.codes_to_host(), codes) and np.array_equal(ix.list_sizes(), sizes)
    assert ix.search_plan(nq, 10, nlist)[:3] == T.ivfpq_plan(nq, nlist, nlist, ix.max_list_tiles) == (nq, 1, nlist * 25)  # one slice: the whole concatenation
    coarse = ivf_ref.int_scores(q, cent)
    S = ivfpq_ref.scores(q, coarse, lists, codes, cb)
    S.setflags(write=False)
    masks, q_filter, allowed = _filter(n, nq)
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    off = _offset(S)
    label = f"dsub={dsub} dim={dim} {dtype} nq={nq}"
    pl = ivfpq_ref.probe(coarse, nlist)[0]
    assert len({tuple(r) for r in pl.tolist()}) > 1  # the lists follow each other in several orders
    _assert_exact(ix.search(q, 10, nlist), ivfpq_ref.search(S, lists, pl, 10, doc_base=BASE), label)
    _assert_exact(ix.search(q, 10, nlist, filter=flt, q_filter=q_filter), ivfpq_ref.search(S, lists, pl, 10, allowed=allowed, doc_base=BASE), label + " filtered")
    exp = ivfpq_ref.search(S, lists, pl, 1024, score_offset=off, doc_base=BASE)
    assert (exp[2] == 1024).all()
    _assert_exact(ix.search(q, 1024, nlist, score_offset=float(off)), exp, label + " offset")
    pl2 = ivfpq_ref.probe(coarse, 2)[0]  # two lists a query: walks of another length, still one slice
    assert ix.search_plan(nq, 100, 2)[1] == 1
    _assert_exact(ix.search(q, 100, 2, score_offset=float(off)), ivfpq_ref.search(S, lists, pl2, 100, score_offset=off, doc_base=BASE), label + " nprobe=2")


@pytest.mark.parametrize("dsub,dim,dtype,nq,nprobe", T.IVFPQ_PASS_CASES)
def test_ivfpq_second_pass(dsub, dim, dtype, nq, nprobe):
    import sparse_rx
    cent, lists, x, cb, q = tq._data(np.random.default_rng(nq), T.IVFPQ_SIZES, dim, dsub, nq=nq)
    n, nlist, first = len(x), len(cent), T.PASS
    ix = tq._build(cent, lists, x, cb, dsub, dtype, doc_base=BASE)
    assert ix.search_plan(nq, 10, nprobe)[0] == first < nq
    codes = ivfpq_ref.codes(x, lists, cent, dtype, cb)
    assert np.array_equal(ix.codes_to_host(), codes)
    coarse = ivf_ref.int_scores(q, cent)
    S = ivfpq_ref.scores(q, coarse, lists, codes, cb)
    masks, q_filter, allowed = _filter(n, nq)
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    off = _offset(S)
    pl = ivfpq_ref.probe(coarse, nprobe)[0]
    exp = ivfpq_ref.search(S, lists, pl, 10, doc_base=BASE)
    _assert_exact(ix.search(q, 10, nprobe), exp, "two passes")
    assert (q_filter[first:] != q_filter[: nq - first]).all()
    _assert_exact(ix.search(q, 10, nprobe, filter=flt, q_filter=q_filter), ivfpq_ref.search(S, lists, pl, 10, allowed=allowed, doc_base=BASE), "two passes, filtered")
    given = _given_lists(nq, nprobe, nlist)
    given[3::5, 0] = nlist  # out of range
    assert (given[first:] != given[: nq - first]).any(axis=1).all()
    want = ivfpq_ref.search(S, lists, given, 1024, score_offset=off, doc_base=BASE)
    _assert_exact(ix.search(q, 1024, nprobe, score_offset=float(off), probe_list=given), want, "two passes, given lists")
    _assert_exact(ix.search(q[first: first + 1], 10, nprobe), tuple(a[first: first + 1] for a in exp), "query 1024 alone")
    _assert_exact(ix.search(q[first: first + 1], 1024, nprobe, score_offset=float(off), probe_list=given[first: first + 1]),
                  tuple(a[first: first + 1] for a in want), "query 1024 alone, given lists")


_PREPARE = {}


def _prepare_world():
    if not _PREPARE:
        sizes = T.ivfpq_prepare_sizes()
        cent, lists, x, cb, q = tq._data(np.random.default_rng(1024), sizes, 16, 4, nq=3)
        ix = tq._build(cent, lists, x, cb, 4, "f16", doc_base=BASE)
        codes = ivfpq_ref.codes(x, lists, cent, "f16", cb)
        assert np.array_equal(ix.codes_to_host(), codes) and np.array_equal(ix.list_sizes(), sizes) and ix.max_list_tiles == 2
        coarse = ivf_ref.int_scores(q, cent)
        S = ivfpq_ref.scores(q, coarse, lists, codes, cb)
        S.setflags(write=False)
        _PREPARE["w"] = (ix, lists, q, coarse, S)
    return _PREPARE["w"]


@pytest.mark.parametrize("nprobe", [p for (p,) in T.IVFPQ_PREPARE_CASES])
def test_ivfpq_prepare_over_many_slots(nprobe):
    ix, lists, q, coarse, S = _prepare_world()
    nlist, nq = ix.nlist, len(q)
    assert ix.search_plan(nq, 1024, nprobe)[:3] == T.ivfpq_plan(nq, nlist, nprobe, 2)
    off = _offset(S)
    pl = ivfpq_ref.probe(coarse, nprobe)[0]
    exp = ivfpq_ref.search(S, lists, pl, 1024, score_offset=off, doc_base=BASE)
    assert (exp[2] > 0).all()
    _assert_exact(ix.search(q, 1024, nprobe, score_offset=float(off)), exp, f"nprobe={nprobe}")
    _assert_exact(ix.search(q, 10, nprobe), ivfpq_ref.search(S, lists, pl, 10, doc_base=BASE), f"nprobe={nprobe} k=10")
    # a caller's rows: a permutation of the lists, and in the highest slots padding, a repeat, a list out of range and a long list
    rng = np.random.default_rng(nprobe)
    given = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int32)
    given[:, -1], given[:, -2], given[:, -3], given[:, -6] = -1, given[:, 0], nlist, nlist + 7
    given[0, -4], given[1, -1], given[2, -5] = 97, 194, -1
    want = ivfpq_ref.search(S, lists, given, 1024, score_offset=off, doc_base=BASE)
    assert (want[2] > 0).all()
    _assert_exact(ix.search(q, 1024, nprobe, score_offset=float(off), probe_list=given), want, f"nprobe={nprobe} given lists")


_IVFPQ_SCORER = {}


@pytest.mark.parametrize("dsub,dim,dtype,m", T.IVFPQ_SCORER_CASES)
def test_ivfpq_scorer_chunks(dsub, dim, dtype, m):
    if (dsub, dim, dtype) not in _IVFPQ_SCORER:
        cent, lists, x, cb, q = tq._data(np.random.default_rng(dim + dsub), T.IVFPQ_SIZES, dim, dsub, nq=3)
        ix = tq._build(cent, lists, x, cb, dsub, dtype, doc_base=BASE)
        codes = ivfpq_ref.codes(x, lists, cent, dtype, cb)
        assert np.array_equal(ix.codes_to_host(), codes)
        _IVFPQ_SCORER[dsub, dim, dtype] = (ix, q, ivfpq_ref.scores(q, ivf_ref.int_scores(q, cent), lists, codes, cb), len(x))
    ix, q, S, n = _IVFPQ_SCORER[dsub, dim, dtype]
    _check_scorer(ix, q, S, n, m, "ivfpq")
