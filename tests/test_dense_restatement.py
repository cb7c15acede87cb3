"""The dense side's restatements (tests/parity.py) on the CPU: the f32 / u8 score kernels' summation order against the
reference's similarity (to the tolerance its BLAS allows) and against a literal per-lane transcription of the kernel; the
fast top-k against np_oracle.dense_topk; the float64 form of the INT8 oracle against its int32 form; the dispatch
arithmetic (QB, splits, sample, S1, workspace layout) on hand-computed cases and against the library's own
srx_dense_workspace_bytes / srx_dense_f32_workspace_bytes; and the dense entry points' argument checks, which return
before anything touches a device."""
import numpy as np
import pytest

import sparse_rx
from oracle import np_oracle
from parity import (dense_f32_ws_bytes, dense_plan, dense_qb, dense_rows_scores, dense_s1, dense_sample, dense_splits,
                    dense_topk_rows, dense_ws)
from sparse_rx import _capi


def _kernel_transcription(rows, q, scale_min=None, score_offset=0.0):
    """srx_dense_f32_scores_kernel / srx_dense_u8_scores_kernel for one query, written out lane by lane (slow: a few docs)."""
    f = np.float32
    dim = len(q)
    out = []
    for d in range(len(rows)):
        lanes = []
        for lane in range(64):
            a = f(0.0)
            for i in range(16):
                if i < dim // 64:
                    r = f(rows[d][lane + 64 * i])
                    if scale_min is not None:
                        r = f(f(r * f(scale_min[2 * d])) + f(scale_min[2 * d + 1]))
                    a = f(a + f(r * f(q[lane + 64 * i])))
                else:
                    a = f(a + f(f(0.0) * f(0.0)))
            lanes.append(a)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [f(lanes[lane] + lanes[lane ^ o]) for lane in range(64)]
        out.append(f(lanes[0] + f(score_offset)) if scale_min is None else lanes[0])
    return np.array(out, f)


def test_dense_rows_scores_is_the_kernel_order():
    rng = np.random.default_rng(11)
    for dim in (64, 192, 1024):
        emb = (rng.standard_normal((6, dim)) * 10.0 ** rng.integers(-3, 4, (6, dim))).astype(np.float32)
        emb[2] = -emb[1]
        emb[3] = 0.0
        q = rng.standard_normal((2, dim)).astype(np.float32)
        got = dense_rows_scores(emb, q, score_offset=np.float32(0.75))
        for j in range(2):
            assert np.array_equal(got[j].view(np.uint32), _kernel_transcription(emb, q[j], score_offset=0.75).view(np.uint32)), dim
        u8 = rng.integers(0, 256, (5, dim)).astype(np.uint8)
        sm = np.stack([rng.random(5) * 0.02 + 1e-4, -rng.random(5)], axis=1).astype(np.float32).reshape(-1)  # negative mins
        got = dense_rows_scores(u8, q, scale_min=sm)
        for j in range(2):
            assert np.array_equal(got[j].view(np.uint32), _kernel_transcription(u8, q[j], scale_min=sm).view(np.uint32)), dim


def test_dense_rows_scores_pinned_to_reference():
    """Restatement A against the reference's own expressions: the float64 product (f32 path) and
    np_oracle.uint8_asymmetric_similarities (u8 path), to the 1e-5 that the reference's BLAS allows -- and it differs from the
    float64-rounded value in the last bits for a visible share of entries, so a bit-exact check against it bites."""
    rng = np.random.default_rng(12)
    for dim in (64, 384, 1024):
        emb = rng.standard_normal((3000, dim)).astype(np.float32)
        emb /= np.linalg.norm(emb, axis=1, keepdims=True)
        q = rng.standard_normal((5, dim)).astype(np.float32)
        got = dense_rows_scores(emb, q)
        exact = q.astype(np.float64) @ emb.astype(np.float64).T
        tol = 1e-5 * (np.abs(q.astype(np.float64)) @ np.abs(emb.astype(np.float64)).T)
        assert np.all(np.abs(got - exact) <= tol), dim
        share = np.mean(got.view(np.uint32) != exact.astype(np.float32).view(np.uint32))
        assert share > 0.2, (dim, share)
        off = np.float32(3.5)
        shifted = dense_rows_scores(emb, q, score_offset=off)
        assert np.array_equal(shifted.view(np.uint32), (got + off).view(np.uint32))

        c8, cs = sparse_rx.quantize_asymmetric(rng.standard_normal((2000, dim)).astype(np.float32))
        qq = [sparse_rx.quantize_query_asymmetric(x) for x in rng.standard_normal((4, dim)).astype(np.float32)]
        q8, qs = np.stack([a for a, _ in qq]), np.stack([b for _, b in qq])
        qf = np.stack([sparse_rx.dense.dequantize_query_asymmetric(a, b) for a, b in qq])
        got = dense_rows_scores(c8, qf, scale_min=cs)
        ref = np_oracle.uint8_asymmetric_similarities(q8, qs, c8, cs)
        n = len(c8)
        doc = c8.astype(np.float32) * cs[0:2 * n:2, None] + cs[1:2 * n:2, None]
        tol = 1e-5 * (np.abs(qf.astype(np.float64)) @ np.abs(doc.astype(np.float64)).T) + 1e-30
        assert np.all(np.abs(got.astype(np.float64) - ref) <= tol), dim
        share = np.mean(got.view(np.uint32) != ref.view(np.uint32))
        assert share > 0.2, (dim, share)


def test_dense_topk_rows_matches_oracle():
    rng = np.random.default_rng(13)
    for n, nq in ((1, 3), (5, 4), (40, 6), (3000, 5)):
        s = rng.integers(-5, 6, (nq, n)).astype(np.float32) * np.float32(0.25)  # few distinct values: ties everywhere
        s[0] = -1.0
        if nq > 3:
            s[3] = rng.standard_normal(n).astype(np.float32)
        for k in (1, 2, n, n + 3, 128, 1024):
            got = dense_topk_rows(s, k)
            exp = np_oracle.dense_topk(s, k)
            for g, e in zip(got, exp):
                assert g.dtype == e.dtype and np.array_equal(g, e), (n, k)


def test_int8_similarities_float64_dot_is_exact():
    """np_oracle.int8_similarities takes the dot as a float64 matmul: bit-identical to the int32 form, at the extremes too."""
    rng = np.random.default_rng(14)
    for dim in (32, 1024):
        c = rng.integers(-128, 128, (300, dim)).astype(np.int8)
        q = rng.integers(-128, 128, (7, dim)).astype(np.int8)
        c[0], c[1], c[2] = -128, 127, -127
        q[0], q[1] = -128, 127
        cs = (rng.random(300) + 0.01).astype(np.float32)
        qs = (rng.random(7) + 0.01).astype(np.float32) / 127
        dots = q.astype(np.int32) @ c.astype(np.int32).T
        assert dots[0, 0] == dim * 128 * 128 and dots[1, 1] == dim * 127 * 127
        exp = ((dots.astype(np.float64) * qs.astype(np.float64)[:, None]) * cs.astype(np.float64)[None, :]).astype(np.float32)
        got = np_oracle.int8_similarities(q, c, qs, cs)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), dim


def test_dense_dispatch_arithmetic():
    assert dense_qb(20_001) == 1024 and dense_qb(1_048_576) == 1024 and dense_qb(1_048_577) == 992
    assert dense_qb(1_100_001) == 960 and dense_qb(4_000_000) == 256 and dense_qb(10 ** 9) == 32
    assert dense_splits(49_953, 130, 100) == 3 and dense_splits(20_001, 1, 100) == 1 and dense_splits(300_000, 4, 10) == 18
    assert dense_splits(300_000, 4, 1024) == 4 and dense_splits(10 ** 8, 1, 1) == 512 * 4
    assert dense_sample(65_535, 10) == 0 and dense_sample(65_536, 10) == 4096 and dense_sample(100_001, 10) == 4096
    assert dense_sample(65_600, 100) == 16384 and dense_sample(65_535 + 1, 100) == 16384
    assert dense_sample(65_536, 1024) == 16384 and dense_sample(65_000 + 535, 1024) == 0
    # one round just above n = 4 S: S1 = sqrt(16 384 n) rounds up past n / 2 (256-doc workgroups for KS <= 12, 128 above)
    assert dense_s1(65_600, 16384, 384) == (65_600, False) and dense_s1(65_600, 16384, 512) == (65_600, False)
    assert dense_s1(100_001, 4096, 384) == (20_480, False) and dense_s1(100_001, 4096, 512) == (20_352, False)
    # chip rounding: sqrt(S n) reaches 512 workgroups (65 536 docs for KS > 12, 131 072 for KS <= 12)
    assert dense_s1(300_000, 16384, 512) == (131_072, True) and dense_s1(300_000, 16384, 384) == (70_144, False)
    assert dense_s1(1_100_001, 16384, 32) == (262_144, True)
    p = dense_plan(1030, 1_100_001, 100, 32)
    assert (p["QB"], p["passes"], p["path"], p["rounds"], p["chip"]) == (960, 2, "filtered", 2, True)
    p = dense_plan(1029, 20_001, 100, 64)
    assert (p["QB"], p["passes"], p["path"], p["ns"]) == (1024, 2, "matrix", 1)


def test_dense_workspace_restatement_matches_library():
    """dense_ws / dense_f32_ws_bytes against the library: the score region pins QB, the candidate buffers the path."""
    L = _capi.lib()
    for n_docs in (1, 5, 33, 20_001, 49_953, 65_535, 65_536, 65_537, 65_600, 100_001, 300_000, 1_048_576, 1_100_001, 4_000_000):
        for nq in (0, 1, 31, 33, 130, 1024, 1029, 5000):
            for k in (1, 10, 100, 129, 1000, 1024):
                assert dense_ws(nq, n_docs, k)["bytes"] == L.srx_dense_workspace_bytes(nq, n_docs, k), (nq, n_docs, k)
                assert dense_f32_ws_bytes(nq, n_docs, k) == L.srx_dense_f32_workspace_bytes(nq, n_docs, k), (nq, n_docs, k)


def _i8(L, fn, n_docs=10, dim=64, nq=1, k=5, doc_base=0, corpus=1 << 20, queries=1 << 22, ws=1 << 27, ws_bytes=1 << 40):
    return getattr(L, fn)(0, corpus, 1 << 21, n_docs, dim, queries, 1 << 23, nq, k, doc_base, 1 << 24, 1 << 25, 1 << 26, ws, ws_bytes, None)


def _rows(L, fn, n_docs=10, dim=64, nq=1, k=5, doc_base=0, ws=1 << 27, ws_bytes=1 << 40):
    if fn == "srx_dense_search_f32":
        return L.srx_dense_search_f32(0, 1 << 20, n_docs, dim, 1 << 22, nq, k, doc_base, 1 << 24, 1 << 25, 1 << 26, ws, ws_bytes, None, 0.0)
    return L.srx_dense_search_u8(0, 1 << 20, 1 << 21, n_docs, dim, 1 << 22, nq, k, doc_base, 1 << 24, 1 << 25, 1 << 26, ws, ws_bytes, None)


@pytest.mark.parametrize("fn", ["srx_dense_search_i8", "srx_dense_search_i8_packed"])
def test_dense_i8_argument_checks(fn):
    L = _capi.lib()

    def rejects(rc, code, text):
        assert rc == code and text in L.srx_last_error(), (rc, L.srx_last_error())

    for k in (0, 1025):
        rejects(_i8(L, fn, k=k), -1, b"1 <= k <= 1024")
    assert L.srx_dense_workspace_bytes(1, 10, 0) == -1 and L.srx_dense_workspace_bytes(1, 10, 1025) == -1
    for dim in (0, 48, 1000, 1056):
        rejects(_i8(L, fn, dim=dim), -1, b"multiple of 32")
    rejects(_i8(L, fn, n_docs=10, doc_base=(1 << 31) - 1 - 10), -1, b"fit int32")
    rejects(_i8(L, fn, doc_base=-1), -1, b"fit int32")
    rejects(_i8(L, fn, corpus=(1 << 20) + 8), -1, b"aligned")
    rejects(_i8(L, fn, queries=(1 << 22) + 4), -1, b"aligned")
    for nq, n_docs, k in ((1, 10, 5), (130, 100_001, 10), (1029, 20_001, 1024)):
        need = L.srx_dense_workspace_bytes(nq, n_docs, k)
        rejects(_i8(L, fn, n_docs=n_docs, nq=nq, k=k, ws_bytes=need - 1), -3, b"workspace too small")
        rejects(_i8(L, fn, n_docs=n_docs, nq=nq, k=k, ws=None, ws_bytes=need), -3, b"workspace too small")
    assert _i8(L, fn, nq=0, ws=None, ws_bytes=0) == 0  # an empty batch is done before the device is touched
    assert L.srx_dense_pack_i8(0, 1 << 20, 10, 96, (1 << 21) + 4, None) == -1 and b"aligned" in L.srx_last_error()
    assert L.srx_dense_pack_i8(0, 1 << 20, 0, 96, 1 << 21, None) == -1 and L.srx_dense_pack_i8(0, 1 << 20, 10, 1056, 1 << 21, None) == -1


@pytest.mark.parametrize("fn", ["srx_dense_search_f32", "srx_dense_search_u8"])
def test_dense_rows_argument_checks(fn):
    L = _capi.lib()

    def rejects(rc, code, text):
        assert rc == code and text in L.srx_last_error(), (rc, L.srx_last_error())

    for k in (0, 1025):
        rejects(_rows(L, fn, k=k), -1, b"1 <= k <= 1024")
    assert L.srx_dense_f32_workspace_bytes(1, 10, 0) == -1 and L.srx_dense_f32_workspace_bytes(1, 10, 1025) == -1
    for dim in (0, 32, 96, 1000, 1088):
        rejects(_rows(L, fn, dim=dim), -1, b"multiple of 64")
    rejects(_rows(L, fn, n_docs=10, doc_base=(1 << 31) - 1 - 10), -1, b"fit int32")
    rejects(_rows(L, fn, doc_base=-1), -1, b"fit int32")
    for nq, n_docs, k in ((1, 10, 5), (9, 300_000, 10), (5, 3001, 1024)):
        need = L.srx_dense_f32_workspace_bytes(nq, n_docs, k)
        rejects(_rows(L, fn, n_docs=n_docs, nq=nq, k=k, ws_bytes=need - 1), -3, b"workspace too small")
    assert _rows(L, fn, nq=0, ws=None, ws_bytes=0) == 0
