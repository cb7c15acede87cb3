"""Oracle parity for every compiled path of the dense kernels (csrc/dense.hip), bit for bit.

The INT8 search is not one code path: srx_dense_i8_scores_kernel<KS> and srx_dense_i8_filter_kernel<KS> are built once per
row length (KS = dim / 32, each with its own staging schedule); corpora of 65 536 docs and more go through a threshold
sample and one or two filter rounds, smaller ones through the score matrix; batches above QB queries run in passes that
re-use the workspace; a query whose candidate buffer overflows is re-ranked through the score matrix.  Every case is
labelled with its dispatch (tests/parity.py: dense_plan, pinned to the library through srx_dense_workspace_bytes) and
asserts that it lands where it was written for; the overflow flags and survivor counts are read out of the workspace at
the restated offsets.  Counts, score bits and ids must equal the oracle's (np_oracle.int8_similarities, ranked score
desc, doc asc).  The f32 / u8 kernels sum in a fixed order without contraction: they are compared bit for bit with
parity.dense_rows_scores, the restatement of that order (pinned to the reference in test_dense_restatement.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import np_oracle  # noqa: E402  (checker only)
from parity import (DENSE_DIMS, dense_f32_ws_bytes, dense_ks_params, dense_plan, dense_plan_label, dense_rows_scores,  # noqa: E402
                    dense_sample, dense_topk_rows, dense_ws)

pytestmark = pytest.mark.gpu

DOC_BASE = 1000


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    return sparse_rx._capi.lib()


def _pinned(L, nq, n_docs, k, dim, **expect):
    """The restated dispatch of a case, checked against the library (workspace size) and against what the case is for."""
    p = dense_plan(nq, n_docs, k, dim)
    assert dense_ws(nq, n_docs, k)["bytes"] == L.srx_dense_workspace_bytes(nq, n_docs, k), f"restated dense_ws drifted (nq={nq} n={n_docs} k={k})"
    for key, want in expect.items():
        assert p[key] == want, f"nq={nq} n={n_docs} k={k} dim={dim}: {key} = {p[key]}, the case was written for {want}"
    return p


def _ws_i32(ix, off, count):
    """int32 words of the index's workspace (as the last pass of its last search left it)."""
    return ix._ws[off: off + 4 * count].cpu().numpy().view(np.int32)


def _any_ovf(ix, nq, n_docs, k):
    return int(_ws_i32(ix, dense_ws(nq, n_docs, k)["any_ovf"], 1)[0])


def _oracle(q, qs, c, cs, k, base=DOC_BASE):
    d, s, n = dense_topk_rows(np_oracle.int8_similarities(q, c, qs, cs), k)
    return np.where(d >= 0, d + base, -1).astype(np.int32), s, n


def _assert_rows(got, exp, label):
    d, s, n = got
    ed, es, en = exp
    assert np.array_equal(n, en), f"{label}: counts differ"
    assert np.array_equal(s.view(np.uint32), es.view(np.uint32)), f"{label}: scores differ"
    assert np.array_equal(d, ed), f"{label}: ids differ"


def _rows(exp, sel):
    return tuple(x[sel] for x in exp)


def _rand_i8(rng, shape):
    return rng.integers(-127, 128, shape, dtype=np.int8)


def _scales(rng, n):
    return (rng.random(n) + 0.01).astype(np.float32)


# ---- INT8: every KS on both paths, packed and row-major -----------------------------------------------------------------
# (dim, path) -> (n_docs, k).  n_docs = 1 or 31 (mod 32): a partial last doc tile.  Filtered cases alternate between two
# rounds (100 001 docs, k = 10) and one (65 567 docs, k = 100: S = 16 384 and S1 rounds up past n / 2).
def _ks_case(dim, path):
    even = DENSE_DIMS.index(dim) % 2 == 0
    if path == "matrix":
        return (49_953, 100) if even else (40_031, 100)
    return (100_001, 10) if even else (65_567, 100)


KS_CASES = [(dim, path) for dim in DENSE_DIMS for path in ("matrix", "filtered")]


def _ks_id(case):
    dim, path = case
    n_docs, k = _ks_case(dim, path)
    return f"dim{dim}-" + dense_plan_label(dense_plan(130, n_docs, k, dim), k)


@pytest.mark.parametrize("case", KS_CASES, ids=[_ks_id(c) for c in KS_CASES])
def test_int8_every_ks(lib, case):
    import sparse_rx
    dim, path = case
    n_docs, k = _ks_case(dim, path)
    rounds = 0 if path == "matrix" else (2 if n_docs == 100_001 else 1)
    rng = np.random.default_rng(1000 + dim + (path == "filtered"))
    c = _rand_i8(rng, (n_docs, dim))
    c[5] = c[6]
    c[n_docs - 1] = c[0]  # exact ties, one of them in the partial last tile
    cs = _scales(rng, n_docs)
    cs[n_docs - 1] = cs[0]
    q, qs = _rand_i8(rng, (130, dim)), _scales(rng, 130) / 127
    exp = _oracle(q, qs, c, cs, k)
    for packed in (True, False):
        ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE, packed=packed)
        for nq in (130, 32, 1):  # five query tiles (the last one partial), one full tile, one query
            _pinned(lib, nq, n_docs, k, dim, path=path, rounds=rounds, passes=1)
            _assert_rows(ix.search(q[:nq], qs[:nq], k), _rows(exp, slice(0, nq)), f"dim {dim} {path} packed={packed} nq={nq}")
            if path == "filtered":
                assert _any_ovf(ix, nq, n_docs, k) == 0, "no query should have needed the fallback"
        del ix


ODD_CASES = [(200, 30_017, 100, "matrix"), (300, 65_537, 10, "filtered"), (1000, 65_567, 100, "filtered")]


@pytest.mark.parametrize("dim,n_docs,k,path", ODD_CASES, ids=[f"dim{c[0]}-{c[3]}" for c in ODD_CASES])
def test_int8_padded_dims(lib, dim, n_docs, k, path):
    """Row lengths between the instantiations: DenseInt8Index pads corpus and queries with zeros (dense._pad_dim)."""
    import sparse_rx
    rng = np.random.default_rng(dim)
    c, cs = _rand_i8(rng, (n_docs, dim)), _scales(rng, n_docs)
    q, qs = _rand_i8(rng, (70, dim)), _scales(rng, 70) / 127
    exp = _oracle(q, qs, c, cs, k)
    for packed in (True, False):
        ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE, packed=packed)
        assert ix.dim_pad == sparse_rx.dense._pad_dim(dim) and ix.dim_pad > dim
        _pinned(lib, 70, n_docs, k, ix.dim_pad, path=path)
        _assert_rows(ix.search(q, qs, k), exp, f"dim {dim} packed={packed}")


# ---- INT8: filter rounds with S1 rounded to whole rounds of the chip ------------------------------------------------------
def test_int8_chip_rounded_first_round_long_rows(lib):
    """KS 16 (128 docs per workgroup): sqrt(S n) = 70 110 >= 65 536, so the first round takes 131 072 docs."""
    import sparse_rx
    dim, n_docs, nq, k = 512, 300_000, 40, 100
    p = _pinned(lib, nq, n_docs, k, dim, path="filtered", rounds=2, chip=True, S1=131_072)
    rng = np.random.default_rng(512)
    c, cs = _rand_i8(rng, (n_docs, dim)), _scales(rng, n_docs)
    q, qs = _rand_i8(rng, (nq, dim)), _scales(rng, nq) / 127
    exp = _oracle(q, qs, c, cs, k)
    ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE)
    _assert_rows(ix.search(q, qs, k), exp, dense_plan_label(p, k))
    assert _any_ovf(ix, nq, n_docs, k) == 0


# ---- INT8: several query passes over one workspace ------------------------------------------------------------------------
def test_int8_two_passes_matrix(lib):
    import sparse_rx
    dim, n_docs, nq, k = 64, 20_001, 1029, 100
    p = _pinned(lib, nq, n_docs, k, dim, path="matrix", QB=1024, passes=2)
    rng = np.random.default_rng(64)
    c, cs = _rand_i8(rng, (n_docs, dim)), _scales(rng, n_docs)
    q, qs = _rand_i8(rng, (nq, dim)), _scales(rng, nq) / 127
    exp = _oracle(q, qs, c, cs, k)
    for packed in (True, False):
        ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE, packed=packed)
        _assert_rows(ix.search(q, qs, k), exp, dense_plan_label(p, k) + f" packed={packed}")


def test_int8_two_passes_filtered_overflow_in_second_pass(lib):
    """1 029 queries = 1 024 + 5: the second pass re-clears the counters and flags and gates the fallback by itself.  Query
    1 026 ties at its top score with ~68 500 docs (column 0 = 100 there, the query is 127 e0): its candidate buffer
    overflows and only it goes through the score matrix; the queries around it do not overflow, in either pass."""
    import sparse_rx
    dim, n_docs, nq, k = 32, 80_001, 1029, 10
    p = _pinned(lib, nq, n_docs, k, dim, path="filtered", QB=1024, passes=2)
    rng = np.random.default_rng(32)
    c = _rand_i8(rng, (n_docs, dim))
    c[:, 0] = 100
    c[::7, 0] = rng.integers(-127, 100, len(c[::7]))  # below the tie: the tie is the top score of query 1 026
    cs = np.ones(n_docs, np.float32)
    q, qs = _rand_i8(rng, (nq, dim)), np.full(nq, 1.0 / 127, np.float32)
    q[1026] = 0
    q[1026, 0] = 127
    assert (c[:, 0] == 100).sum() > 65_536
    sel = np.unique(np.concatenate([[0, 1023, 1024, 1026, 1028], rng.choice(nq, 6, replace=False)]))
    exp = _oracle(q[sel], qs[sel], c, cs, k)
    for packed in (True, False):
        ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE, packed=packed)
        d, s, n = ix.search(q, qs, k)
        _assert_rows((d[sel], s[sel], n[sel]), exp, dense_plan_label(p, k) + f" packed={packed}")
        w = dense_ws(nq, n_docs, k)
        ovf = _ws_i32(ix, w["ovf"], w["qb"])  # the second pass's flags: queries 1 024 .. 1 028 in its first five
        assert ovf[2] == 1 and ovf.sum() == 1 and _any_ovf(ix, nq, n_docs, k) == 1, ovf[:8]
        ix.search(q[:1024], qs[:1024], k)
        assert _any_ovf(ix, 1024, n_docs, k) == 0, "the first pass alone must not overflow"


def test_int8_two_passes_qb_below_1024(lib):
    """1.1 M docs: QB = 960 (the score matrix of the fallback within 4 GiB), 1 030 queries in two passes; S1 = 262 144 is
    rounded to whole rounds of the chip at KS 1 (256 docs per workgroup).  Sampled rows around the pass boundary."""
    import sparse_rx
    dim, n_docs, nq, k = 32, 1_100_001, 1030, 100
    p = _pinned(lib, nq, n_docs, k, dim, path="filtered", QB=960, passes=2, rounds=2, chip=True, S1=262_144)
    rng = np.random.default_rng(1100)
    c, cs = _rand_i8(rng, (n_docs, dim)), _scales(rng, n_docs)
    q, qs = _rand_i8(rng, (nq, dim)), _scales(rng, nq) / 127
    sel = np.unique(np.concatenate([[0, 959, 960, 1029], rng.choice(nq, 4, replace=False)]))
    exp = _oracle(q[sel], qs[sel], c, cs, k)
    ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE)
    d, s, n = ix.search(q, qs, k)
    _assert_rows((d[sel], s[sel], n[sel]), exp, dense_plan_label(p, k))
    assert _any_ovf(ix, nq, n_docs, k) == 0


# ---- INT8: survivor pressure at every KS ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DENSE_DIMS, ids=[f"ks{d // 32}-cb{dense_ks_params(d)['DENSE_CB']}" for d in DENSE_DIMS])
def test_int8_survivor_pressure(lib, dim):
    """Three distinct rows (40 / 30 / 30 % of the corpus): each query's scores take three values, its top group ties at the
    threshold and passes whole -- more survivors in one 32-query x 32 DT-doc tile than the wave's list holds (DENSE_CB), so
    entries go straight to the buffer inside a tile and the list is flushed mid-loop on every tile.  The survivor counts
    in the workspace must be the top groups' sizes: nothing lost, nothing appended twice."""
    import sparse_rx
    n_docs, nq, k = 65_537, 64, 1000
    _pinned(lib, nq, n_docs, k, dim, path="filtered", passes=1)
    rng = np.random.default_rng(2000 + dim)
    pats = _rand_i8(rng, (3, dim))
    c = pats[rng.choice(3, size=n_docs, p=[0.4, 0.3, 0.3])]
    cs = np.ones(n_docs, np.float32)
    q, qs = _rand_i8(rng, (nq, dim)), np.full(nq, 1.0 / 127, np.float32)
    sims = np_oracle.int8_similarities(q, c, qs, cs)
    top = sims.max(axis=1)
    group = sims == top[:, None]
    surv = group & (top[:, None] > 0)
    S = dense_sample(n_docs, k)
    assert np.all(group[:, :S].sum(axis=1) >= k)  # the k-th best of the sample is the top score: the group passes whole
    prm = dense_ks_params(dim)
    t = 32 * prm["DT"]
    per_tile = surv[:, : n_docs // t * t].reshape(nq // 32, 32, -1, t).sum(axis=(1, 3))
    assert per_tile.max() > prm["DENSE_CB"], (per_tile.max(), prm)
    d, s, n = dense_topk_rows(sims, k)
    exp = (np.where(d >= 0, d + DOC_BASE, -1).astype(np.int32), s, n)
    w = dense_ws(nq, n_docs, k)
    for packed in (True, False):
        ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE, packed=packed)
        _assert_rows(ix.search(q, qs, k), exp, f"ks {dim // 32} packed={packed}")
        cnt = _ws_i32(ix, w["buf_cnt"], nq * 32)[::32]
        assert np.array_equal(cnt, surv.sum(axis=1)), (cnt[:8], surv.sum(axis=1)[:8])
        assert _any_ovf(ix, nq, n_docs, k) == 0


# ---- INT8: k edges, few positive scores, tiny corpora ---------------------------------------------------------------------
@pytest.mark.parametrize("path", ["matrix", "filtered"])
def test_int8_k_edges(lib, path):
    """k = 1, 2, 127 / 128 / 129, 1 023 / 1 024 on one corpus; query 0 has 37 positive scores (rows padded -1 / 0 past
    them), query 1 none."""
    import sparse_rx
    dim, n_docs = (96, 30_017) if path == "matrix" else (64, 65_537)
    rng = np.random.default_rng(3000 + dim)
    c, cs = _rand_i8(rng, (n_docs, dim)), _scales(rng, n_docs)
    c[:, 0] = -100
    c[rng.choice(n_docs, 37, replace=False), 0] = 100
    q, qs = _rand_i8(rng, (40, dim)), _scales(rng, 40) / 127
    q[0] = 0
    q[0, 0] = 127
    q[1] = 0
    exp = _oracle(q, qs, c, cs, 1024)
    assert exp[2][0] == 37 and exp[2][1] == 0
    ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE)
    for k in (1, 2, 127, 128, 129, 1023, 1024):
        p = _pinned(lib, 40, n_docs, k, dim, path=path, passes=1)
        e = (exp[0][:, :k], exp[1][:, :k], np.minimum(exp[2], k))
        _assert_rows(ix.search(q, qs, k), e, dense_plan_label(p, k))


@pytest.mark.parametrize("n_docs", [1, 5, 31, 33])
def test_int8_tiny_corpus_k_above_n_docs(lib, n_docs):
    import sparse_rx
    rng = np.random.default_rng(4000 + n_docs)
    for dim in (32, 1024):
        c, cs = _rand_i8(rng, (n_docs, dim)), _scales(rng, n_docs)
        q, qs = _rand_i8(rng, (3, dim)), _scales(rng, 3) / 127
        for packed in (True, False):
            ix = sparse_rx.DenseInt8Index(c, cs, doc_base=DOC_BASE, packed=packed)
            for k in sorted({1, n_docs, 64, 1024}):
                _pinned(lib, 3, n_docs, k, dim, path="matrix")
                _assert_rows(ix.search(q, qs, k), _oracle(q, qs, c, cs, k), f"n {n_docs} dim {dim} k {k} packed={packed}")


# ---- INT8: a row length without an instantiation is refused, the outputs stay as they were --------------------------------------
def test_int8_uninstantiated_ks_is_refused(lib):
    """dim = 160 is a multiple of 32 but KS = 5 is not compiled (DenseInt8Index would pad it to 192; the C ABI does not):
    -1 and the list of row lengths, and the three output arrays keep their sentinels.  This pins the refusal, not its place in
    the driver: a library that enqueues the query packing before it refuses never touches the outputs either and passes too."""
    import torch
    dim, n_docs, nq, k = 160, 64, 1, 5
    assert dim not in DENSE_DIMS and dim % 32 == 0
    dev = torch.device("cuda:0")
    c = torch.ones(lib.srx_dense_packed_bytes(n_docs, dim), dtype=torch.int8, device=dev)  # n_docs x dim in either order
    cs = torch.ones(n_docs, dtype=torch.float32, device=dev)
    q = torch.ones(nq * dim, dtype=torch.int8, device=dev)
    qs = torch.ones(nq, dtype=torch.float32, device=dev)
    ws_bytes = lib.srx_dense_workspace_bytes(nq, n_docs, k)
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    for entry in ("srx_dense_search_i8", "srx_dense_search_i8_packed"):
        od = torch.full((nq * k,), -7, dtype=torch.int32, device=dev)
        os_ = torch.full((nq * k,), -3.5, dtype=torch.float32, device=dev)
        oc = torch.full((nq,), -9, dtype=torch.int32, device=dev)
        rc = getattr(lib, entry)(0, c.data_ptr(), cs.data_ptr(), n_docs, dim, q.data_ptr(), qs.data_ptr(), nq, k, DOC_BASE,
                                 od.data_ptr(), os_.data_ptr(), oc.data_ptr(), ws.data_ptr(), ws_bytes,
                                 torch.cuda.current_stream().cuda_stream)
        msg = lib.srx_last_error().decode()
        torch.cuda.synchronize()
        assert rc == -1, entry
        assert "dim must be 32, 64, 96, 128, 192, 256, 384, 512, 768 or 1024" in msg, (entry, msg)
        assert (od.cpu().numpy() == -7).all() and (os_.cpu().numpy() == np.float32(-3.5)).all() and (oc.cpu().numpy() == -9).all(), entry


# ---- srx_dense_pack_i8 against the layout of include/sparse_rx.h -------------------------------------------------------------
def test_pack_i8_layout(lib):
    """rows[32 T + (l & 31)][32 s + 16 (l >> 5) ..] at packed + ((T dim / 32 + s) 64 + l) 16, zeros past n_rows."""
    import torch
    rng = np.random.default_rng(5000)
    stream = torch.cuda.current_stream().cuda_stream
    for dim in DENSE_DIMS:
        for n_rows in (1, 31, 32, 33, 4133):
            rows = _rand_i8(rng, (n_rows, dim))
            nbytes = lib.srx_dense_packed_bytes(n_rows, dim)
            T = (n_rows + 31) // 32
            assert nbytes == T * 32 * dim
            dev = torch.as_tensor(rows, device="cuda:0")
            out = torch.full((nbytes,), 0x55, dtype=torch.int8, device="cuda:0")  # the zero rows must be written
            assert lib.srx_dense_pack_i8(0, dev.data_ptr(), n_rows, dim, out.data_ptr(), stream) == 0
            torch.cuda.synchronize()
            full = np.zeros((T * 32, dim), np.int8)
            full[:n_rows] = rows
            exp = full.reshape(T, 32, dim // 32, 2, 16).transpose(0, 2, 3, 1, 4).reshape(-1)  # [T][s][h][r][16 bytes]
            assert np.array_equal(out.cpu().numpy(), exp), (dim, n_rows)


# ---- f32 / u8: bit for bit against the restated summation order ---------------------------------------------------------------
# every slice count 1 .. 16 (dim 64 .. 1 024), nq cycling through 1, 3, 4, 5, 9 (passes of four), k through 1 / 10 / 128 /
# 129 / 1 024; one split on 3 001 docs, 18 splits on 300 000 docs (k = 10), 4 at k = 1 024.
ROWS_CASES = [(kind, dim, 3001, (1, 3, 4, 5, 9)[i % 5], (1, 10, 128, 129, 1024)[i % 5])
              for kind in ("f32", "u8") for i, dim in enumerate(range(64, 1025, 64))]
ROWS_CASES += [("f32", 64, 300_000, 5, 10), ("u8", 128, 300_000, 3, 10), ("f32", 192, 300_000, 4, 1024)]


def _rows_id(case):
    kind, dim, n_docs, nq, k = case
    from parity import dense_splits
    return f"{kind}-s{dim // 64}-n{n_docs}-nq{nq}-k{k}-ns{dense_splits(n_docs, 4, k)}"


@pytest.mark.parametrize("case", ROWS_CASES, ids=[_rows_id(c) for c in ROWS_CASES])
def test_rows_kernels_bit_exact(lib, case):
    import torch

    import sparse_rx
    kind, dim, n_docs, nq, k = case
    assert dense_f32_ws_bytes(nq, n_docs, k) == lib.srx_dense_f32_workspace_bytes(nq, n_docs, k)
    rng = np.random.default_rng(6000 + dim + n_docs)
    emb = rng.standard_normal((n_docs, dim)).astype(np.float32)
    emb[:, 0] = np.abs(emb[:, 0]) + 0.5
    emb[7] = emb[3]
    emb[n_docs - 1] = emb[0]  # duplicate rows: exact ties, ranked doc-ascending
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    if nq > 1:
        q[-1] = 0
        q[-1, 0] = -1.0  # every score negative: count 0
    if kind == "f32":
        ix = sparse_rx.DenseF32Index(emb, doc_base=DOC_BASE)
        runs = [(0.0, ix.search(q, k)), (0.37, ix.search(q, k, score_offset=0.37))]
        restated = [(off, dense_rows_scores(emb, q, score_offset=np.float32(off))) for off, _ in runs]
    else:
        c8, cs = sparse_rx.quantize_asymmetric(emb)  # mins < 0
        cs[14:16] = cs[6:8]  # the reader's [2 d], [2 d + 1]: doc 7 duplicates doc 3 exactly
        assert np.array_equal(c8[7], c8[3]) and np.any(cs[1::2] < 0)
        ix = sparse_rx.DenseUint8Index(c8, cs, doc_base=DOC_BASE)
        d, s, n = ix.search_device(torch.as_tensor(q, device=ix.device), k)
        torch.cuda.synchronize()
        runs = [(0.0, (d.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()))]
        restated = [(0.0, dense_rows_scores(c8, q, scale_min=cs))]
    for (off, got), (_, sc) in zip(runs, restated):
        ed, es, en = np_oracle.dense_topk(sc, k) if n_docs < 10_000 else dense_topk_rows(sc, k)
        exp = (np.where(ed >= 0, ed + DOC_BASE, -1).astype(np.int32), es, en)
        if kind == "f32" and nq > 1:
            assert en[-1] == 0
        _assert_rows(got, exp, f"{_rows_id(case)} offset={off}")


def test_service_min_score_second_pass_picks_restated_rows(lib):
    """search_by_vector with fewer than k positive scores and min_score <= 0: the shifted pass (score_offset = 1.001 x
    the Cauchy-Schwarz bound) picks k rows at the resolution of ulp(offset); they must be exactly the rows the restated
    shifted ranking picks (ties doc-ascending), re-scored with np.dot and re-ranked stably."""
    import sparse_rx
    rng = np.random.default_rng(7000)
    n_docs, dim, k = 4000, 96, 300
    emb = rng.standard_normal((n_docs, dim)).astype(np.float32)
    emb[:, 0] = -np.abs(emb[:, 0]) - 0.5
    emb[11] = emb[10]
    qv = rng.standard_normal(dim).astype(np.float32) * np.float32(0.3)
    qv[0] = 6.0
    n_pos = int((np.dot(emb, qv) > 0).sum())
    assert 0 < n_pos < k
    svc = sparse_rx.RetrievalService()
    svc.set_embeddings(emb)
    got = svc.search_by_vector(qv, k=k, min_score=-1e30)
    offset = float(np.linalg.norm(qv.astype(np.float64))) * svc._dense.max_row_norm() * 1.001 + 1e-30  # service.py's shift
    ep = np.zeros((n_docs, 128), np.float32)
    ep[:, :dim] = emb
    qp = np.zeros((1, 128), np.float32)
    qp[0, :dim] = qv
    sd, ss, sn = np_oracle.dense_topk(dense_rows_scores(ep, qp, score_offset=np.float32(offset)), k)
    assert sn[0] == k
    idx = sd[0].astype(np.int64)
    sc = np.dot(emb[idx], qv).astype(np.float32)
    order = np.argsort(-sc, kind="stable")
    assert [r["doc_id"] for r in got] == [str(int(i)) for i in idx[order]]
    assert [r["score"] for r in got] == [float(x) for x in sc[order]]
