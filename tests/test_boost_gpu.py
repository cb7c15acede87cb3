"""Field-value boosts on the GPU (include/boost/sparse_rx_boost.h).  Expected rows are never the engine's own: the restatement
(tests/boost_ref.py) on the columns, clauses and lists a call was given.  Every comparison is exact -- doc ids, positions, counts
and the BITS of the scores --, and every output buffer is pre-filled with 0x7f bytes so that a word the kernel does not write
shows.  tests/test_boost_cpu.py shows that these inputs give other bits under a fused multiply-add."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import boost_ref  # noqa: E402
from boost_ref import ABS, F32, MULTIPLY, N_DOCS, DOC_BASE, REPLACE, SCORE_MAX, SCORE_MIN, SCORE_MULTIPLY, SCORE_SUM, SUM, f32, f32_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
GARBAGE = 0x7F7F7F7F


class _Table:
    """The columns of boost_ref.table() on the device, as the C call takes them, next to their host arrays"""

    def __init__(self, cols, n_docs=N_DOCS, doc_base=DOC_BASE):
        import torch
        from sparse_rx import _capi
        from sparse_rx.filter import pack_masks
        self.cols, self.n_docs, self.doc_base = cols, n_docs, doc_base
        self.keep = []
        self.desc = (_capi.FieldColDesc * len(cols))()
        for i, (typ, data, valid) in enumerate(cols):
            d_t = torch.from_numpy(np.ascontiguousarray(data)).to(DEVICE)
            v_t = None if valid is None else torch.from_numpy(pack_masks(np.asarray(valid, dtype=bool)).view(np.int32).copy()).to(DEVICE).reshape(-1)
            self.keep += [d_t, v_t]
            self.desc[i].data, self.desc[i].valid, self.desc[i].type = d_t.data_ptr(), None if v_t is None else v_t.data_ptr(), typ

    def run(self, clauses, knots, score_mode, boost_mode, doc, score, count, k, carry=None, pos=True, stream=None):
        """The C call on garbage-filled outputs -> host (doc, score bits, count, pos | None)"""
        import torch
        from sparse_rx import _capi
        up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEVICE)
        nq, m = doc.shape
        d_t, s_t, c_t = up(doc, np.int32), up(score, np.float32), up(count, np.int32)
        kc = 0 if carry is None else carry[0].shape[1]
        cd_t, cs_t, cc_t = (None, None, None) if carry is None else (up(carry[0], np.int32), up(carry[1], np.float32), up(carry[2], np.int32))
        cl_t = torch.from_numpy(boost_ref.clause_array(clauses).view(np.uint8).copy()).to(DEVICE)
        kn_t = up(knots, np.float32)
        o_doc, o_score, o_pos = (torch.full((nq, k), GARBAGE, dtype=torch.int32, device=DEVICE) for _ in range(3))
        o_count = torch.full((nq,), GARBAGE, dtype=torch.int32, device=DEVICE)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        rc = _capi.lib().srx_boost_topk(0, self.desc, len(self.cols), self.n_docs, self.doc_base, ptr(cl_t), len(clauses), ptr(kn_t), len(knots), score_mode,
                                        boost_mode, ptr(d_t), ptr(s_t), ptr(c_t), ptr(cd_t), ptr(cs_t), ptr(cc_t), nq, m, kc, k, ptr(o_doc), ptr(o_score),
                                        ptr(o_count), ptr(o_pos) if pos else None, sp)
        _capi.check(rc, "srx_boost_topk")
        torch.cuda.synchronize()
        return (o_doc.cpu().numpy(), o_score.cpu().numpy().view(np.uint32), o_count.cpu().numpy(), o_pos.cpu().numpy() if pos else None)

    def check(self, clauses, knots, score_mode, boost_mode, doc, score, count, k, carry=None, what=None):
        got = self.run(clauses, knots, score_mode, boost_mode, doc, score, count, k, carry)
        cr = (None, None, None) if carry is None else carry
        want = boost_ref.boost_topk(self.cols, self.n_docs, self.doc_base, clauses, knots, score_mode, boost_mode, doc, score, count, k, *cr)
        for g, w, name in zip(got, want, ("doc", "score bits", "count", "pos")):
            assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())
        return want


@pytest.fixture(scope="module")
def tab():
    return _Table(boost_ref.table())


# ---- 1. geometry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 1024, 2048])
def test_geometry(tab, m):
    half = max(1, m // 2)
    seen = set()
    for kc_of in (0, 1, "k"):
        for k_of in (1, half, "all"):
            kc = kc_of if kc_of != "k" else (m if k_of == "all" else k_of)
            if m + kc > 2048:
                continue
            k = m + kc if k_of == "all" else k_of
            if (kc, k) in seen:
                continue
            seen.add((kc, k))
            clauses, knots, d, s, c, carry = boost_ref.bit_case(1000 + m + 7 * kc + k, nq=3, m=m, kc=kc)
            tab.check(clauses, knots, SCORE_MULTIPLY, MULTIPLY, d, s, c, k, carry, what=(m, kc, k))
    assert len(seen) >= 3


@pytest.mark.parametrize("nq", [0, 1, 3, 300])
def test_query_counts(tab, nq):
    clauses, knots, d, s, c, carry = boost_ref.bit_case(50 + nq, nq=nq, m=65, kc=3)
    want = tab.check(clauses, knots, SCORE_SUM, SUM, d, s, c, 20, carry)
    assert want[0].shape == (nq, 20)
    if nq == 300:
        assert (want[2] <= 3).any() and (want[2] == 20).any()  # a count of -3 leaves only the carry; most rows fill


@pytest.mark.parametrize("col", [0, 1, 2])
def test_each_column_type_alone(tab, col):
    """I32 with a validity row, I64 without one, F32 with one: a clause with and one without ABS over the same column, and no count"""
    rng = np.random.default_rng(70 + col)
    clauses, knots = boost_ref.curves(rng, 2, cols_used=(col,))
    clauses[0]["flags"], clauses[1]["flags"] = 0, ABS
    d, s, _, _ = boost_ref.lists(rng, 4, 300, 0)
    want = tab.check(clauses, knots, SCORE_MULTIPLY, MULTIPLY, d, s, None, 300)
    assert (want[2] > 250).all()
    # the same column without its validity row: other bits wherever a doc was missing
    typ, data, valid = tab.cols[col]
    bare = _Table([(typ, data, None)])
    for c in clauses:
        c["col"] = 0
    got = bare.check(clauses, knots, SCORE_MULTIPLY, MULTIPLY, d, s, None, 300)
    assert (valid is None) == bool(np.array_equal(got[1], want[1]))


# ---- 2. edges of the values and of the curve --------------------------------------------------------------------------------------------
def _planted(n=64):
    doc = (np.arange(n, dtype=np.int32) + DOC_BASE)[None]
    return doc, np.full((1, n), 1.5, dtype=np.float32)


def test_value_edges(tab):
    doc, score = _planted()
    knots = np.array([0.5, 2.0, 1.0, 3.0, 0.25], dtype=np.float32)
    i64_origins = (0, 2 ** 53, -(2 ** 53), 2 ** 63 - 1, -(2 ** 63), 1_650_000_000)
    for origin in i64_origins:  # beyond 2^53 the double conversion rounds; INT64_MIN - INT64_MAX overflows nothing in double
        for flags in (0, ABS):
            for inv in (f32(1e-18), f32(1.0 / 86400), f32(1.0), f32(1e30)):
                cl = [dict(col=1, flags=flags, origin=origin, inv_step=inv, weight=f32(1), missing=f32(7), knot0=0, n_seg=4)]
                tab.check(cl, knots, SCORE_MULTIPLY, MULTIPLY, doc, score, None, 64, what=("i64", origin, flags, float(inv)))
    for origin in (0.0, -0.0, 1.0, np.inf, -np.inf, 1e-45, 3.4028235e38):  # inf - inf is a NaN offset: t > 0 fails, y[0]
        for flags in (0, ABS):
            for inv in (f32(1e-45), f32(1e-38), f32(0.5), f32(3e38)):  # denormal steps and products, and ones that overflow
                cl = [dict(col=2, flags=flags, origin=f32_bits(origin), inv_step=inv, weight=f32(1), missing=f32(7), knot0=0, n_seg=4)]
                tab.check(cl, knots, SCORE_MULTIPLY, MULTIPLY, doc, score, None, 64, what=("f32", origin, flags, float(inv)))
    # the NaNs of the F32 column (docs 2 and 12) and its invalid doc 13 take `missing`; -0.0 and +0.0 the same knot
    cl = [dict(col=2, flags=0, origin=f32_bits(-1.0), inv_step=f32(1.0), weight=f32(1), missing=f32(7), knot0=0, n_seg=4)]
    want = tab.check(cl, knots, SCORE_MULTIPLY, REPLACE, doc, score, None, 64)
    by_doc = dict(zip(want[0][0].tolist(), want[1][0].view(np.float32).tolist()))
    assert by_doc[DOC_BASE + 2] == by_doc[DOC_BASE + 12] == by_doc[DOC_BASE + 13] == 7.0 and by_doc[DOC_BASE + 3] == by_doc[DOC_BASE + 4] == 2.0
    # I32 at both ends of its type, and its invalid doc 6
    for origin in (0, 2 ** 31 - 1, -(2 ** 31), 2 ** 40):
        cl = [dict(col=0, flags=ABS, origin=origin, inv_step=f32(1e-9), weight=f32(-2), missing=f32(7), knot0=1, n_seg=3)]
        tab.check(cl, knots, SCORE_MULTIPLY, SUM, doc, score, None, 64, what=("i32", origin))


def test_curve_edges(tab):
    """t exactly on the knots, one ulp below n_seg, negative offsets without ABS, n_seg = 1 and 256"""
    rng = np.random.default_rng(5)
    for n_seg in (1, 256):
        knots = (rng.random(n_seg + 3) + 0.1).astype(np.float32)
        below = np.nextafter(f32(n_seg), f32(0))
        vals = np.concatenate([np.arange(-3, n_seg + 3, dtype=np.float32), [below, np.nextafter(f32(n_seg), f32(np.inf)), 0.5, n_seg - 0.5, np.float32(1e-45)]])
        col = np.zeros(1000, dtype=np.float32)
        col[: len(vals)] = vals
        t = _Table([(F32, col, None)], n_docs=1000, doc_base=17)
        doc = (np.arange(len(vals), dtype=np.int32) + 17)[None]
        score = np.ones((1, len(vals)), dtype=np.float32)
        for flags in (0, ABS):
            cl = [dict(col=0, flags=flags, origin=f32_bits(0.0), inv_step=f32(1.0), weight=f32(1), missing=f32(0), knot0=1, n_seg=n_seg)]
            want = t.check(cl, knots, SCORE_MULTIPLY, REPLACE, doc, score, None, len(vals), what=(n_seg, flags))
            f = dict(zip(want[0][0].tolist(), want[1][0].view(np.float32).tolist()))
            y = knots[1: n_seg + 2]
            for j in range(n_seg + 1):  # a value on knot j is knot j
                assert f[17 + 3 + j] == y[j]
            assert f[17 + 3 + n_seg + 1] == f[17 + 3 + n_seg + 2] == y[n_seg]  # beyond the last knot: flat
            assert f[17] == (y[min(3, n_seg)] if flags else y[0])              # x = -3: y[0] without ABS


@pytest.mark.parametrize("boost_mode", [MULTIPLY, SUM, REPLACE])
@pytest.mark.parametrize("score_mode", [SCORE_MULTIPLY, SCORE_SUM, SCORE_MAX, SCORE_MIN])
def test_mode_pairs(tab, score_mode, boost_mode):
    for n_clauses, weights in ((1, None), (8, None), (8, (-1.5, 0.75, -0.25))):
        rng = np.random.default_rng(100 * score_mode + 10 * boost_mode + n_clauses)
        clauses, knots = boost_ref.curves(rng, n_clauses, weights=weights)
        d, s, c, carry = boost_ref.lists(rng, 3, 200, 9)
        tab.check(clauses, knots, score_mode, boost_mode, d, s, c, 50, carry, what=(n_clauses, weights))


# ---- 3. the order ------------------------------------------------------------------------------------------------------------------------
def test_ties_nans_and_zeros(tab):
    rng = np.random.default_rng(9)
    knots = np.array([0.75, 0.75], dtype=np.float32)
    const = [dict(col=0, flags=0, origin=0, inv_step=f32(1), weight=f32(1), missing=f32(0.75), knot0=0, n_seg=1)]
    d, s, _, _ = boost_ref.lists(rng, 3, 500, 0, special=False)
    want = tab.check(const, knots, SCORE_MULTIPLY, REPLACE, d, s, None, 500)  # every score ties: doc-ascending
    for q in range(3):
        n = want[2][q]
        assert n > 490 and (np.diff(want[0][q, :n]) > 0).all() and (want[1][q, :n] == f32_bits(0.75)).all()
    # NaN raw scores come last (behind -inf), among themselves by doc id, and are stored canonical
    s2 = s.copy()
    s2[:, ::7] = np.nan
    s2[:, 1::7] = np.array([0xFFC12345], dtype=np.uint32).view(np.float32)[0]
    s2[:, 2::7] = -np.inf
    s2[:, 3::7] = np.inf
    want = tab.check(const, knots, SCORE_MULTIPLY, MULTIPLY, d, s2, None, 500)
    n = want[2][0]
    tail = want[1][0, :n] == boost_ref.NAN_BITS
    assert tail.sum() > 100 and not tail[: n - tail.sum()].any() and (np.diff(want[0][0, :n][tail]) > 0).all()
    # +0 ranks ahead of -0: raw +-0 under MULTIPLY by a positive constant, and under SUM with a zero curve
    s3 = np.where(np.arange(500) % 2 == 0, 0.0, -0.0).astype(np.float32)[None].repeat(3, 0)
    want = tab.check(const, knots, SCORE_MULTIPLY, MULTIPLY, d, s3, None, 500)
    n = want[2][1]
    bits = want[1][1, :n]
    assert (bits[: (bits == 0).sum()] == 0).all() and (bits[(bits == 0).sum():] == 0x80000000).all() and 0 < (bits == 0).sum() < n
    # a carry keeps its bits, NaN payloads included, and ranks by them
    carry = (d[:, :40].copy(), s2[:, :40].copy(), None)
    tab.check(const, knots, SCORE_MULTIPLY, MULTIPLY, d[:, 40:], s[:, 40:], None, 460, carry)


def test_optional_pos_side_stream_and_bad_clauses(tab):
    import torch
    clauses, knots, d, s, c, carry = boost_ref.bit_case(77, nq=5, m=100, kc=10)
    want = boost_ref.boost_topk(tab.cols, N_DOCS, DOC_BASE, clauses, knots, 0, 0, d, s, c, 30, *carry)
    got = tab.run(clauses, knots, 0, 0, d, s, c, 30, carry, pos=False)
    assert got[3] is None and all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = tab.run(clauses, knots, 0, 0, d, s, c, 30, carry, stream=side)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # a clause that names no column, or whose knots leave the table, reads nothing: its factor is `missing`
    for bad in (dict(col=3), dict(col=-1), dict(knot0=len(knots) - 2, n_seg=2), dict(knot0=-1), dict(n_seg=0), dict(n_seg=2 ** 31 - 1)):
        cl = [dict(clauses[0], **bad)]
        got = tab.run(cl, knots, 0, REPLACE, d, s, c, 30, carry)
        fresh = got[3] >= 10  # positions of candidates: their new score is weight * missing
        assert fresh.any() and (got[1][fresh] == f32_bits(f32(cl[0]["weight"]) * f32(cl[0]["missing"]))).all()


def test_refusals_on_the_gpu_machine():
    import test_boost_cpu
    test_boost_cpu.refusals()


# ---- 4. the FieldTable doors ---------------------------------------------------------------------------------------------------------
def test_field_table_doors():
    import torch
    from sparse_rx import BoostResolver, FieldTable
    from sparse_rx.fields import host_columns
    rng = np.random.default_rng(21)
    n = 5000
    date = rng.integers(1_600_000_000, 1_700_000_000, n).astype(np.int64)
    votes = np.ma.masked_array(rng.integers(0, 3000, n).astype(np.int32), mask=rng.random(n) < 0.1)
    price = (rng.random(n) * 100).astype(np.float32)
    given = {"date": date, "votes": votes, "price": price, "tags": [["a"]] * n}
    host = host_columns(given)
    table = FieldTable.from_columns(given, device=DEVICE, doc_base=300)
    spec = {"functions": [{"decay": {"field": "date", "origin": 1_650_000_000, "scale": 86400 * 60}},
                          {"field_value": {"field": "votes", "lo": 0, "hi": 3000, "modifier": "log1p", "missing": 0.5, "weight": 0.25}},
                          {"decay": {"field": "price", "origin": 20.0, "scale": 10.0, "kind": "linear", "offset": 2.5}}],
            "score_mode": "sum", "boost_mode": "multiply"}
    res = BoostResolver(table.columns, spec)
    ref_cols = [(host[nm].type, host[nm].data, host[nm].valid) for nm in res.names]
    doc = np.stack([rng.permutation(n + 40)[:700] + 280 for _ in range(4)]).astype(np.int32)
    score = (rng.random(doc.shape) * 9 + 0.1).astype(np.float32)
    count = np.array([700, 0, 333, 9999], dtype=np.int32)
    carry = (doc[:, :50].copy(), score[:, :50].copy(), np.array([50, 3, -1, 60], dtype=np.int32))
    want = boost_ref.boost_topk(ref_cols, n, 300, list(res.clauses), res.knots, res.score_mode, res.boost_mode, doc[:, 50:], score[:, 50:], count, 100, *carry)
    got = table.boost(spec, doc[:, 50:], score[:, 50:], count, 100, carry=carry, want_pos=True)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w)
    assert len(table.boost(res, doc, score, None, 10)) == 3
    with pytest.raises(ValueError, match="set column"):
        table.boost({"functions": [{"decay": {"field": "tags", "origin": 1, "scale": 1}}]}, doc, score, None, 10)
    with pytest.raises(ValueError, match="at most 2048"):
        table.boost(spec, np.zeros((1, 2040), np.int32), np.zeros((1, 2040), np.float32), None, 10, carry=(np.zeros((1, 9), np.int32), np.zeros((1, 9), np.float32)))
    with pytest.raises(ValueError, match=r"k must be in \[1, m \+ kc = 700\]"):
        table.boost(spec, doc, score, None, 701)
    with pytest.raises(ValueError, match="is on cpu"):
        table.boost_device(res.names, torch.zeros((3, 40), dtype=torch.uint8), torch.zeros(600), 0, 0, torch.from_numpy(doc), torch.from_numpy(score), None, 5)
    table.close()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------
def _ref_boost_dict(results, res, columns, row, top_k):
    """boost_ref over result dicts: {qid: [(doc id, boosted score)]}"""
    ref_cols = [(columns[nm].type, columns[nm].data, columns[nm].valid) for nm in res.names]
    n = len(next(iter(columns.values())))
    out = {}
    for q, hits in results.items():
        ids = list(hits)
        if not ids:
            out[q] = []
            continue
        d = np.asarray([[row[i] for i in ids]], dtype=np.int32)
        s = np.asarray([[hits[i] for i in ids]], dtype=np.float32)
        k = min(top_k, len(ids))
        od, ob, oc, op = boost_ref.boost_topk(ref_cols, n, 0, list(res.clauses), res.knots, res.score_mode, res.boost_mode, d, s, None, k)
        out[q] = [(ids[p], float(b)) for p, b in zip(op[0, : oc[0]], ob[0, : oc[0]].view(np.float32))]
    return out


def test_search_bm25_boost_is_exact_over_the_complete_ranking(tmp_path):
    import sparse_rx
    from sparse_rx.fields import host_columns
    n_all, n = 2000, 900
    rng = np.random.default_rng(45)
    corpus = {f"d{i}": {"text": " ".join(["common"] * (1 + i % 3) * (i < n) + ["rare"] * (i % 5 == 0 and i < n) + ["pad"] * int(rng.integers(1, 40)))}
              for i in range(n_all)}
    queries = {"qa": "common rare", "qb": "common", "blank": "  "}
    row = {d: i for i, d in enumerate(corpus)}
    date = rng.integers(1_640_000_000, 1_660_000_000, n_all).astype(np.int64)
    flag = (np.arange(n_all) % 3 != 0).astype(np.int32)
    fields = {"date": date, "flag": flag, "tags": [["a"]] * n_all}
    columns = host_columns(fields)
    spec = {"functions": [{"decay": {"field": "date", "origin": 1_650_000_000, "scale": 86400 * 20, "kind": "gauss"}}]}
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=8)
    svc.build_bm25_index(corpus)
    with pytest.raises(ValueError, match=r"search_bm25\(boost=\.\.\.\) needs the docs' fields"):
        svc.search_bm25(queries, top_k=5, boost=spec)
    svc.set_doc_fields(fields)
    res = sparse_rx.BoostResolver(columns, spec)
    full = svc.search_bm25(queries, top_k=n_all)
    assert len(full["qa"]) == n and full["blank"] == {}
    plain = svc.search_bm25(queries, top_k=5)
    cached = len(svc.query_cache)
    svc._be.boost_page = 8  # pages of 8 rows: dozens of rounds per query
    for k in (5, 10):
        got = svc.search_bm25(queries, top_k=k, boost=spec)
        want = _ref_boost_dict(full, res, columns, row, k)
        for q in queries:
            assert list(got[q].items()) == want[q], (k, q)
        assert len(got["qa"]) == k and got["blank"] == {}
    assert list(got["qa"]) != list(full["qa"])[:10]  # the decay reordered the ranking
    # under where= and excluded_docs=: the boosted ranking of the allowed docs
    got = svc.search_bm25(queries, top_k=5, boost=spec, where={"must": [{"field": "flag", "eq": 1}]})
    want = _ref_boost_dict({q: {d: s for d, s in full[q].items() if flag[row[d]] == 1} for q in full}, res, columns, row, 5)
    assert all(list(got[q].items()) == want[q] for q in queries)
    out = list(full["qa"])[:30]
    got = svc.search_bm25(queries, top_k=5, boost=spec, excluded_docs=out)
    want = _ref_boost_dict({q: {d: s for d, s in full[q].items() if d not in set(out)} for q in full}, res, columns, row, 5)
    assert all(list(got[q].items()) == want[q] for q in queries)
    # a depth limit: the boosted top of the rows read
    got = svc.search_bm25(queries, top_k=5, boost=spec, boost_depth=40)
    want = _ref_boost_dict({q: dict(list(full[q].items())[:40]) for q in full}, res, columns, row, 5)
    assert all(list(got[q].items()) == want[q] for q in queries)
    svc._be.boost_page = 1024
    got = svc.search_bm25(queries, top_k=5, boost=spec)  # one page holds the ranking
    want = _ref_boost_dict(full, res, columns, row, 5)
    assert all(list(got[q].items()) == want[q] for q in queries)
    assert len(svc.query_cache) == cached  # none of these calls read or wrote the cache
    assert svc.search_bm25(queries, top_k=5) == plain == svc.search_bm25(queries, top_k=5, boost=None, boost_depth=3)
    for bad, word in ((dict(collapse_by="flag"), "do not combine"), (dict(top_k=1025), "at most 1024 rows"),
                      (dict(boost={**spec, "boost_mode": "replace"}), "replace"),
                      (dict(boost={"functions": [{"decay": {"field": "tags", "origin": 1, "scale": 1}}]}), "set column")):
        with pytest.raises(ValueError, match=word):
            svc.search_bm25(queries, **{"top_k": 5, "boost": spec, **bad})
    # boost_results over the same dicts, every boost_mode
    for mode in ("multiply", "sum", "replace"):
        sp = {**spec, "boost_mode": mode}
        r2 = sparse_rx.BoostResolver(columns, sp)
        deep = svc.search_bm25(queries, top_k=300)
        for top_k in (None, 7):
            got = svc.boost_results(deep, sp, top_k=top_k)
            want = _ref_boost_dict(deep, r2, columns, row, 300 if top_k is None else top_k)
            assert list(got) == list(deep) and all(list(got[q].items()) == want[q] for q in deep), (mode, top_k)
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.boost_results({"qa": {"no such doc": 1.0}}, spec)
    with pytest.raises(ValueError, match="at most 2048 docs"):
        svc.boost_results({"v": [{"doc_id": f"d{i % n_all}", "score": 1.0} for i in range(2049)]}, spec)
    assert svc.boost_results({}, spec) == {}
    # the registry mirrors go through the same backend functions
    r = sparse_rx.OptimizedBM25Retriever(device=DEVICE, tile_log2=8)
    r.build_index_from_corpus(corpus)
    r.set_doc_fields(fields)
    r._be.boost_page = 8
    rfull = r.search({"qa": queries["qa"]}, top_k=n_all)
    got = r.search({"qa": queries["qa"]}, top_k=5, boost=spec)
    assert list(got["qa"].items()) == _ref_boost_dict(rfull, res, columns, row, 5)["qa"]
    assert list(r.boost_results(rfull, spec, top_k=5)["qa"].items()) == list(got["qa"].items())
    r.close()
    p = sparse_rx.OptimizedRetriever({"type": "bm25"}, device=DEVICE, tile_log2=8, cache_dir=str(tmp_path))
    p.build_index_from_corpus(corpus)
    p.set_doc_fields(fields)
    p._be.boost_page = 8
    pfull = p.search({"qb": queries["qb"]}, top_k=n_all)  # its own accumulation order, its own floats
    got = p.search({"qb": queries["qb"]}, top_k=5, boost=spec)
    assert list(got["qb"].items()) == _ref_boost_dict(pfull, res, columns, row, 5)["qb"]
    p.close()
    svc.close()


def test_search_bm25_boost_with_expansion():
    import sparse_rx
    from sparse_rx.fields import host_columns
    n_all = 600
    rng = np.random.default_rng(46)
    words = [f"w{i}" for i in range(40)]
    corpus = {f"d{i}": {"text": " ".join(rng.choice(words, size=int(rng.integers(5, 30))))} for i in range(n_all)}
    queries = {"q1": "w1 w2", "q2": "w7"}
    fields = {"votes": rng.integers(0, 1000, n_all).astype(np.int32)}
    columns = host_columns(fields)
    spec = {"functions": [{"field_value": {"field": "votes", "lo": 0, "hi": 1000, "modifier": "sqrt", "factor": 0.01}}], "boost_mode": "sum"}
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(corpus)
    svc.set_doc_fields(fields)
    svc.enable_feedback()
    svc._be.boost_page = 16
    kw = dict(expand_docs=5, expand_terms=6)
    full = svc.search_bm25(queries, top_k=n_all, **kw)
    got = svc.search_bm25(queries, top_k=8, boost=spec, **kw)
    want = _ref_boost_dict(full, sparse_rx.BoostResolver(columns, spec), columns, {d: i for i, d in enumerate(corpus)}, 8)
    assert all(list(got[q].items()) == want[q] for q in queries) and all(len(got[q]) == 8 for q in queries)
    svc.close()


@pytest.fixture(scope="module")
def text(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    ids = list(j["corpus"])
    rng = np.random.default_rng(3)
    return j, ids, {"parent": [i // 4 for i in range(len(ids))], "price": (rng.random(len(ids)) * 50).astype(np.float32),
                    "date": rng.integers(0, 10_000, len(ids)).astype(np.int64)}


def test_search_hybrid_boost_equals_the_reference_over_the_pool(text):
    import sparse_rx
    from sparse_rx.fields import host_columns
    j, ids, fields = text
    queries = {q: j["queries"][q] for q in list(j["queries"])[:10]}
    n_docs, dim = len(ids), 64
    rng = np.random.default_rng(47)
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    svc.set_embeddings(rng.standard_normal((n_docs, dim)).astype(np.float32))
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    spec = {"functions": [{"decay": {"field": "date", "origin": 5000, "scale": 1500, "kind": "exp"}},
                          {"decay": {"field": "price", "origin": 10.0, "scale": 8.0, "kind": "linear", "weight": 0.5}}], "score_mode": "max"}
    with pytest.raises(ValueError, match=r"search_hybrid\(boost=\.\.\.\) needs the docs' fields"):
        svc.search_hybrid(queries, vecs, top_k=5, boost=spec)
    svc.set_doc_fields(fields)
    columns, row = host_columns(fields), {d: i for i, d in enumerate(ids)}
    same = lambda a, b: {q: list(v.items()) for q, v in a.items()} == {q: list(v.items()) for q, v in b.items()}
    for extra in (dict(), dict(rescore=True), dict(fusion="rrf"), dict(excluded_docs=ids[:40])):
        for mode in ("multiply", "replace"):
            sp = {**spec, "boost_mode": mode}
            got = svc.search_hybrid(queries, vecs, top_k=5, boost=sp, boost_pool=40, **extra)
            pool = svc.search_hybrid(queries, vecs, top_k=40, **extra)
            want = _ref_boost_dict(pool, sparse_rx.BoostResolver(columns, sp), columns, row, 5)
            assert all(list(got[q].items()) == want[q] for q in queries), (extra, mode)
            assert same(got, svc.boost_results(pool, sp, top_k=5))
    got = svc.search_hybrid(queries, vecs, top_k=5, boost=spec)  # the default pool: min(max(20, 100), 1024, n_docs)
    assert same(got, svc.boost_results(svc.search_hybrid(queries, vecs, top_k=100), spec, top_k=5))
    # then collapse, then MMR: the chain of the public steps
    got = svc.search_hybrid(queries, vecs, top_k=5, boost=spec, boost_pool=40, collapse_by="parent")
    assert same(got, svc.collapse(svc.boost_results(svc.search_hybrid(queries, vecs, top_k=40), spec), "parent", top_k=5))
    got = svc.search_hybrid(queries, vecs, top_k=5, boost=spec, boost_pool=40, mmr_lambda=0.5, mmr_pool=12)
    assert same(got, svc.diversify(svc.boost_results(svc.search_hybrid(queries, vecs, top_k=40), spec, top_k=12), top_k=5, mmr_lambda=0.5))
    # after the late-interaction rerank of the whole pool (boost_pool is then late_pool)
    svc.set_token_embeddings({d: rng.standard_normal((3, 32)).astype(np.float32) for d in ids})
    qt = {q: rng.standard_normal((4, 32)).astype(np.float32) for q in queries}
    got = svc.search_hybrid(queries, vecs, top_k=5, boost=spec, late_query_tokens=qt, late_pool=30)
    assert same(got, svc.boost_results(svc.rerank_late(svc.search_hybrid(queries, vecs, top_k=30), qt, top_k=30), spec, top_k=5))
    with pytest.raises(ValueError, match="boost_pool must be in"):
        svc.search_hybrid(queries, vecs, top_k=5, boost=spec, boost_pool=1025)
    assert same(svc.search_hybrid(queries, vecs, top_k=5, boost=None, boost_pool=7), svc.search_hybrid(queries, vecs, top_k=5))
    svc.close()


def test_search_hybrid_three_stages_equal_the_chain_of_the_public_steps(text):
    """boost + collapse + MMR, and late rerank + boost + collapse: one call = the public doors chained over the pool"""
    import sparse_rx
    j, ids, fields = text
    queries = {q: j["queries"][q] for q in list(j["queries"])[:10]}
    n_docs, dim = len(ids), 64
    rng = np.random.default_rng(48)
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    svc.set_embeddings(rng.standard_normal((n_docs, dim)).astype(np.float32))
    svc.set_doc_fields(fields)
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    spec = {"functions": [{"decay": {"field": "date", "origin": 5000, "scale": 1500, "kind": "exp"}},
                          {"decay": {"field": "price", "origin": 10.0, "scale": 8.0, "kind": "linear", "weight": 0.5}}], "score_mode": "max"}
    same = lambda a, b: {q: list(v.items()) for q, v in a.items()} == {q: list(v.items()) for q, v in b.items()}
    got = svc.search_hybrid(queries, vecs, top_k=5, boost=spec, boost_pool=40, collapse_by="parent", mmr_lambda=0.5, mmr_pool=12)
    assert all(len(v) == 5 for v in got.values())
    assert same(got, svc.diversify(svc.collapse(svc.boost_results(svc.search_hybrid(queries, vecs, top_k=40), spec), "parent", top_k=12), top_k=5,
                                   mmr_lambda=0.5))
    svc.set_token_embeddings({d: rng.standard_normal((3, 32)).astype(np.float32) for d in ids})
    qt = {q: rng.standard_normal((4, 32)).astype(np.float32) for q in queries}
    got = svc.search_hybrid(queries, vecs, top_k=5, boost=spec, collapse_by="parent", late_query_tokens=qt, late_pool=30)
    assert all(len(v) == 5 for v in got.values())
    assert same(got, svc.collapse(svc.boost_results(svc.rerank_late(svc.search_hybrid(queries, vecs, top_k=30), qt, top_k=30), spec), "parent", top_k=5))
    svc.close()
