"""What csrc/build.hip writes on the MI355X against tests/build_ref.py, bit for bit: no tolerances anywhere in this file.

The inputs come from tests/test_build_cpu.py, which asserts without a GPU that each of them holds the edge it is there for.
  test_layout_case          the directed layout cases through DeviceIndex.from_coo: term_ptr, tile_skip, post (the 256 sentinel
                            blocks behind the last run included), post16 (None where a unit exceeds 49 152 docs), n_blocks, nnz,
                            unit_tiles; the same with unit_tiles = 0 against build_ref.auto_unit_tiles
  test_grid_stride_*        inputs larger than one trip of the capped grids, every element compared
  test_tile_skip_direct     srx_build_tile_skip at tile_log2 0 and 30
  test_sum_duplicates_* / test_from_csr_sums_*   the summation order of duplicates
  test_term_bounds_*        a workgroup's second and third term, caller-given ranks, non-finite and signed-zero values
  test_empty_index          an index without postings builds, searches and scores"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import build_ref  # noqa: E402
import test_build_cpu as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()
    return sparse_rx


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


def _from_coo(rx, rows, cols, vals, n_docs, vocab, **kw):
    import torch
    return rx.DeviceIndex.from_coo(_dev(rows), _dev(cols), _dev(vals), torch.ones(vocab, dtype=torch.float32, device="cuda:0"), n_docs,
                                   mode="dot", device="cuda:0", **kw)


def _assert_index_equals(ix, ref, unit_tiles, np_dtype, nnz, label):
    tp, post, skip, nb = ref
    assert (ix.n_blocks, ix.nnz, ix.unit_tiles) == (nb, nnz, unit_tiles), label
    assert np.array_equal(ix.term_ptr.cpu().numpy(), tp), label
    assert np.array_equal(ix.tile_skip.cpu().numpy(), skip), label
    got = ix.post.cpu().numpy()
    assert got.dtype == post.dtype and got.shape == post.shape, label
    bad = np.flatnonzero(got != post)
    assert not len(bad), f"{label}: post differs at {len(bad)} words, first {bad[:6]}: {got[bad[:6]]} != {post[bad[:6]]}"
    if (unit_tiles << ix.tile_log2) > build_ref.UNIT_MAX_DOCS:
        assert ix.post16 is None, label
    else:
        assert ix.post16 is not None, label
        assert np.array_equal(ix.post16.cpu().numpy(), build_ref.compact(post, unit_tiles << ix.tile_log2, np_dtype)), label


@pytest.mark.parametrize("name", list(cases.LAYOUT_BY_NAME))
def test_layout_case(rx, name):
    c = cases.LAYOUT_BY_NAME[name]
    rows, cols, vals = c.coo
    for ut in (c.unit_tiles, 0):
        ix = _from_coo(rx, rows, cols, vals, c.n_docs, c.vocab, val_dtype=c.vd, tile_log2=c.tile_log2, unit_tiles=ut, score_bounds=c.score_bounds)
        try:
            want = ut or build_ref.auto_unit_tiles(c.n_docs, c.vocab, len(rows), c.tile_log2)
            ref = build_ref.layout(rows, cols, vals, c.n_docs, c.vocab, c.tile_log2, want, c.np_dtype)
            _assert_index_equals(ix, ref, want, c.np_dtype, len(rows), f"{name} unit_tiles={ut}")
            if name == cases.SEARCHED_CASE and ut:  # no compact copy: every query is tier 2's, the rows are still the oracle's
                import oracle
                assert ix.post16 is None
                rng = np.random.default_rng(3)
                q_term = np.concatenate([np.sort(rng.choice(c.vocab, 5, replace=False)) for _ in range(12)]).astype(np.int32)
                q = (np.arange(13, dtype=np.int32) * 5, q_term, np.ones(60, np.float32))
                indptr, indices, data = cases.coo_to_csr(rows, cols, vals, c.n_docs)
                exp = oracle.search_batch(indptr, indices, data, None, np.ones(c.vocab, np.float32), *q, 20, mode=oracle.MODE_TFIDF_F32)
                got = ix.search(*q, 20)
                assert exp[2].max() == 20, "the queries must fill their rows"
                assert all(np.array_equal(g.view(np.int32), e.view(np.int32)) for g, e in zip(got, exp)), name
        finally:
            ix.close()


def test_grid_stride_skip_tables_and_scatter(rx):
    """70 001 terms x 64 skip entries = 4 480 064 > 4 194 304 and 4 194 604 postings: the second trip of srx_tile_skip_kernel,
    srx_blocks_skip_kernel and srx_blocks_scatter_kernel, every word compared.  Units of 5 tiles: the 13th is partial."""
    rows, cols, vals = cases.stride_corpus()
    V, n, tl, ut = cases.STRIDE_VOCAB, cases.STRIDE_DOCS, cases.STRIDE_TILE_LOG2, cases.STRIDE_UNIT_TILES
    ix = _from_coo(rx, rows, cols, vals, n, V, tile_log2=tl, unit_tiles=ut, score_bounds=False)
    try:
        assert ix.tile_skip.numel() > build_ref.CAP_SKIP and ix.nnz > build_ref.CAP_SKIP
        _assert_index_equals(ix, build_ref.layout(rows, cols, vals, n, V, tl, ut, np.float32), ut, np.float32, len(rows), "stride")
    finally:
        ix.close()


def test_tile_skip_direct_at_tile_log2_0_and_30(rx):
    """The ABI takes tile_log2 0 .. 30: every doc its own tile, and one tile for everything."""
    import torch
    rng = np.random.default_rng(50)
    V, n_docs = 50, 3_000
    lens = rng.integers(0, 200, V)
    lens[[0, 7]] = (0, n_docs)
    term_ptr = np.zeros(V + 1, np.int64)
    term_ptr[1:] = np.cumsum(lens)
    docs = np.concatenate([np.sort(rng.choice(n_docs, L, replace=False)) for L in lens]).astype(np.int32)
    tp_d, doc_d = _dev(term_ptr), _dev(docs)
    for tl, n_tiles in ((0, n_docs), (30, 1)):
        out = torch.full((V * (n_tiles + 1),), -7, dtype=torch.int32, device="cuda:0")
        rc = rx._capi.lib().srx_build_tile_skip(0, tp_d.data_ptr(), doc_d.data_ptr(), V, n_tiles, tl, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        edges = np.arange(n_tiles + 1, dtype=np.int64) << tl
        exp = np.stack([np.searchsorted(docs[term_ptr[t]:term_ptr[t + 1]], edges, side="left") for t in range(V)]).astype(np.int32)
        assert np.array_equal(out.cpu().numpy().reshape(V, n_tiles + 1), exp), tl


def test_grid_stride_impacts_and_value_edges(rx):
    """2 097 452 postings (srx_impact_kernel's grid covers 2 097 152 per trip): fractional and huge tf, tf = 0, docs of length 0,
    b = 0, b = 1, an avgdl that is no float32 -- the bits of oracle.np_oracle.impacts_f32."""
    import torch
    from oracle import np_oracle
    tf, doc, dl = cases.impact_inputs()
    t = [_dev(x) for x in (tf, doc, dl)]
    for k1, b, avgdl in cases.IMPACT_PARAMS:
        exp = np_oracle.impacts_f32(tf, doc, dl, k1, b, avgdl)
        out = torch.full((len(tf),), -7.0, dtype=torch.float32, device="cuda:0")
        rc = rx._capi.lib().srx_build_impacts(0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(tf), k1, b, avgdl, out.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        bad = np.flatnonzero(out.cpu().numpy().view(np.uint32) != exp.view(np.uint32))
        assert not len(bad), f"k1={k1} b={b} avgdl={avgdl}: {len(bad)} differ, first at {bad[:5]} tf {tf[bad[:5]]} len {dl[doc[bad[:5]]]}"


def test_sum_duplicates_direct_keeps_the_input_order(rx):
    """srx_build_sum_duplicates on 2 097 452 groups (one trip of its grid covers 2 097 152), 4 000 of them long with sums that
    depend on the order (asserted on the CPU): left to right, one float32 rounding per add."""
    import torch
    first, vals, long_at = cases.dup_groups()
    out = torch.full((len(first) - 1,), -7.0, dtype=torch.float32, device="cuda:0")
    f_d, v_d = _dev(first), _dev(vals)
    rc = rx._capi.lib().srx_build_sum_duplicates(0, f_d.data_ptr(), len(first) - 1, v_d.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got, exp = out.cpu().numpy(), build_ref.sum_groups(first, vals)
    bad = np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))
    assert not len(bad), f"{len(bad)} groups differ ({np.isin(bad, long_at).sum()} of them long), first {bad[:5]}: {got[bad[:5]]} != {exp[bad[:5]]}"


def test_from_csr_sums_duplicates_like_scipy(rx):
    """300 (doc, term) pairs listed three times, not adjacent in their rows, with order-dependent sums: the stored blocks are the
    layout of SciPy's summed matrix (the CPU file asserts that SciPy adds in input order and that the order matters)."""
    n_docs, V, indptr, cols, vals = cases.dup_corpus()
    m = cases.dup_corpus_summed().tocoo()
    ix = rx.DeviceIndex.from_csr(indptr, cols, vals, np.ones(V, np.float32), mode="dot", tile_log2=6, unit_tiles=2, score_bounds=False)
    try:
        ref = build_ref.layout(m.row, m.col, m.data, n_docs, V, 6, 2, np.float32)
        _assert_index_equals(ix, ref, 2, np.float32, m.nnz, "duplicates")
    finally:
        ix.close()


# ---- term bounds -----------------------------------------------------------------------------------------------------------
def _bounds_abi(rx, term_ptr, vals, ks):
    """srx_build_term_bounds with the caller's ranks: (out f32[V, nk], neg_flag)."""
    import torch
    V = len(term_ptr) - 1
    tp_d, v_d, ks_d = _dev(np.asarray(term_ptr, np.int64)), _dev(vals), _dev(np.asarray(ks, np.int32))
    out = torch.full((V, len(ks)), -7.0, dtype=torch.float32, device="cuda:0")
    neg = torch.full((1,), 5, dtype=torch.int32, device="cuda:0")
    vt = rx._capi.SRX_VAL_F16 if vals.dtype == np.float16 else rx._capi.SRX_VAL_F32
    rc = rx._capi.lib().srx_build_term_bounds(0, vt, tp_d.data_ptr(), v_d.data_ptr(), V, ks_d.data_ptr(), len(ks), out.data_ptr(), neg.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rx._capi.lib().srx_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(neg.item())


def _assert_bounds(got, exp, label):
    bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
    assert not len(bad), f"{label}: {len(bad)} entries differ, first (term, rank column) {bad[:5].tolist()}: {[float(got[t, j]) for t, j in bad[:5]]} != {[float(exp[t, j]) for t, j in bad[:5]]}"


@pytest.mark.parametrize("vd", ["f32", "f16"])
def test_term_bounds_second_and_third_term_of_a_workgroup(rx, vd):
    """vocab 8 229 > 2 x 4 096 workgroups: workgroup b serves a long term (full list, high threshold), then a short one whose
    values all lie below that threshold, then an empty or all-zero one.  Through the C ABI with ranks of the caller's and through
    DeviceIndex._term_bounds (FINE_KS)."""
    import torch
    term_ptr, vals, b = cases.tb_stride_inputs(np.float32 if vd == "f32" else np.float16)
    ks = [1024, 1, 10]
    got, neg = _bounds_abi(rx, term_ptr, vals, ks)
    assert neg == 0
    _assert_bounds(got, build_ref.term_bounds(term_ptr, vals, ks)[0], f"{vd} ks={ks}")
    fine = rx.DeviceIndex._term_bounds(torch, torch.zeros(1, dtype=torch.int32, device="cuda:0"), _dev(vals), _dev(term_ptr), None, len(term_ptr) - 1)
    _assert_bounds(fine.cpu().numpy(), build_ref.term_bounds(term_ptr, vals, rx.DeviceIndex.FINE_KS)[0], f"{vd} FINE_KS")


@pytest.mark.parametrize("name", list(cases.TB_KS_CASES))
def test_term_bounds_with_the_callers_ranks(rx, name):
    """1 to 64 ranks, unsorted, repeated: lengths K - 1, K, K + 1 and ties that straddle rank K, f32 and f16."""
    ks = cases.TB_KS_CASES[name]
    for dt in (np.float32, np.float16):
        term_ptr, vals, _ = cases.tb_rank_inputs(ks, dt)
        got, neg = _bounds_abi(rx, term_ptr, vals, ks)
        assert neg == 0
        _assert_bounds(got, build_ref.term_bounds(term_ptr, vals, ks)[0], f"{name} {dt.__name__}")


def test_term_bounds_of_special_values(rx):
    """+inf is the largest value and a bound of +inf is returned; a NaN is never counted and raises no flag; -0.0 is a zero
    (bound 0, flag clear); one negative value, however small, raises the flag; fp16 subnormals come back as their exact
    float32 (include/sparse_rx.h, srx_build_term_bounds)."""
    inf, nan = np.inf, np.nan
    terms = [[inf, 1.0, 2.0], [nan, 3.0, nan, 1.0], [-0.0] * 5, [nan], [2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -14, 0.0], [inf, inf, 7.0], []]
    term_ptr = np.concatenate([[0], np.cumsum([len(x) for x in terms])]).astype(np.int64)
    flat = np.asarray([v for x in terms for v in x], np.float32)
    ks = [1, 2, 3, 4]
    exp = np.asarray([[inf, 2, 1, 0], [3, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [2.0 ** -14, 3 * 2.0 ** -24, 2.0 ** -24, 0], [inf, inf, 7, 0],
                      [0, 0, 0, 0]], np.float32)
    assert np.array_equal(build_ref.term_bounds(term_ptr, flat, ks)[0].view(np.uint32), exp.view(np.uint32))
    for dt, tiny in ((np.float32, -1e-30), (np.float16, -(2.0 ** -24))):
        vals = flat.astype(dt)
        got, neg = _bounds_abi(rx, term_ptr, vals, ks)
        _assert_bounds(got, exp, dt.__name__)
        assert neg == 0, "NaN and -0.0 are not negative"
        for at in (0, len(vals) - 1):
            v2 = vals.copy()
            v2[at] = tiny
            assert v2[at] < 0 and _bounds_abi(rx, term_ptr, v2, ks)[1] == 1, (dt, at)


# ---- an index without postings -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bm25", "dot"])
def test_empty_index(rx, mode):
    """A shard whose docs are all empty: it builds; post and post16 are exactly the sentinel blocks; a search returns counts 0 and
    the usual padding (doc -1, score +0); score_docs returns zeros."""
    n_docs, V = 5, 3
    ix = rx.DeviceIndex.from_csr(np.zeros(n_docs + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.ones(V, np.float32),
                                 doc_lengths=np.zeros(n_docs, np.float32), avgdl=1.0, mode=mode, tile_log2=6)
    try:
        assert (ix.nnz, ix.n_blocks) == (0, 0) and ix.fine_bound is None and ix.term_bound is None
        assert ix.unit_tiles == build_ref.auto_unit_tiles(n_docs, V, 0, 6) == 64
        e = np.zeros(0, np.int32)
        tp, post, skip, nb = build_ref.layout(e, e, np.zeros(0, np.float32), n_docs, V, 6, ix.unit_tiles, np.float32)
        assert nb == 0 and not tp.any() and not skip.any()
        _assert_index_equals(ix, (tp, post, skip, nb), ix.unit_tiles, np.float32, 0, f"empty {mode}")
        assert np.array_equal(post.reshape(256, 8)[:, :4], np.repeat(-1 - 32 * (np.arange(256) % 64), 4).reshape(256, 4))
        q = (np.asarray([0, 2, 3], np.int32), np.asarray([0, 2, 1], np.int32), np.ones(3, np.float32))
        d, s, n = ix.search(*q, 10)
        assert np.array_equal(n, [0, 0]) and np.array_equal(d, np.full((2, 10), -1, np.int32)) and not s.view(np.uint32).any()
        sc = ix.score_docs(*q, np.asarray([[0, 4, -1, 7], [1, 2, 3, 4]], np.int32))
        assert sc.shape == (2, 4) and not sc.view(np.uint32).any()
    finally:
        ix.close()
