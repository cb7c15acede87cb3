"""Field-value boosts without a GPU: the fourteenth header and its symbol table, every refusal of the entry point (none reaches a
device), the resolver (Elasticsearch's formulas at the knots, the table's distance from the formula, the F bounds, every
ValueError), boost_deep over a fake search on CPU tensors against the brute force, the refusals of the doors, and the sensitivity
of the GPU bit tests' data to a fused multiply-add."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import boost_ref
import sparse_rx
from sparse_rx import _capi, boost
from sparse_rx.backend import SparseBackend, boost_deep
from sparse_rx.fields import host_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(24)]  # 16-byte aligned addresses, never dereferenced


def test_fourteenth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "boost", "sparse_rx_boost.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef SPARSE_RX_BOOST_H")[1]))
    assert declared == set(_capi.BOOST_SYMBOLS) == {"srx_boost_topk"}
    assert '#include "sparse_rx_fields.h"' in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS, _capi.MMR_SYMBOLS,
              _capi.TERMS_SYMBOLS, _capi.MAXSIM_SYMBOLS, _capi.FIELDS_SYMBOLS, _capi.COLLAPSE_SYMBOLS, _capi.FACET_SYMBOLS, _capi.FEEDBACK_SYMBOLS,
              _capi.ORDER_SYMBOLS)
    for other in others:
        assert not set(_capi.BOOST_SYMBOLS) & set(other)
    assert sum(len(t) for t in others) + len(_capi.BOOST_SYMBOLS) == 74
    assert os.listdir(os.path.join(ROOT, "include", "boost")) == ["sparse_rx_boost.h"]
    assert "boost.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "boost", "sparse_rx_boost.h") in _capi._deps()
    assert "include/boost/sparse_rx_boost.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read().split('"""')[1]
    L = _capi.lib()
    for name, (res, args) in _capi.BOOST_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert len(_capi.BOOST_SYMBOLS["srx_boost_topk"][1]) == len(inspect.signature(_call).parameters) - 1 == 26
    for name, value, ref in (("SRX_BOOST_SCORE_MULTIPLY", 0, "SCORE_MULTIPLY"), ("SRX_BOOST_SCORE_SUM", 1, "SCORE_SUM"), ("SRX_BOOST_SCORE_MAX", 2, "SCORE_MAX"),
                             ("SRX_BOOST_SCORE_MIN", 3, "SCORE_MIN"), ("SRX_BOOST_MULTIPLY", 0, "MULTIPLY"), ("SRX_BOOST_SUM", 1, "SUM"),
                             ("SRX_BOOST_REPLACE", 2, "REPLACE"), ("SRX_BOOST_ABS", 1, "ABS")):
        assert re.search(rf"\b{name} = {value}\b", hdr) and getattr(_capi, name) == value == getattr(boost_ref, ref), name
    for name, value, ref in (("SRX_BOOST_MAX_M", 2048, "MAX_M"), ("SRX_BOOST_MAX_CLAUSES", 8, "MAX_CLAUSES"), ("SRX_BOOST_MAX_COLS", 8, "MAX_COLS"),
                             ("SRX_BOOST_MAX_KNOTS", 1 << 24, "MAX_KNOTS")):
        assert re.search(rf"#define {name} {value}\b", hdr) and getattr(_capi, name) == value == getattr(boost_ref, ref), name
    # the clause struct: 40 bytes, the same offsets in ctypes, in the resolver's dtype and in the restatement's
    assert ctypes.sizeof(_capi.BoostClause) == 40 == boost.CLAUSE_DTYPE.itemsize == boost_ref.CLAUSE_DTYPE.itemsize == boost_ref.CLAUSE_BYTES
    assert "40 bytes" in hdr and boost.CLAUSE_DTYPE == boost_ref.CLAUSE_DTYPE
    for name, _ in _capi.BoostClause._fields_:
        assert getattr(_capi.BoostClause, name).offset == boost.CLAUSE_DTYPE.fields[name][1], name
    assert [n for n, _ in _capi.BoostClause._fields_] == list(boost.CLAUSE_DTYPE.names) == re.findall(
        r"^\s+(?:int32_t|int64_t|float) (\w+);", hdr.split("typedef struct srx_boost_clause")[1].split("}")[0], re.M)
    assert (boost_ref.I32, boost_ref.I64, boost_ref.F32, boost_ref.SET64) == (_capi.SRX_FIELD_I32, _capi.SRX_FIELD_I64, _capi.SRX_FIELD_F32,
                                                                             _capi.SRX_FIELD_SET64)
    assert boost.SCORE_MODES == {"multiply": 0, "sum": 1, "max": 2, "min": 3} and boost.BOOST_MODES == {"multiply": 0, "sum": 1, "replace": 2}
    assert sparse_rx.boost_deep is boost_deep is boost.boost_deep and {"boost", "BoostResolver", "BoostFn", "boost_deep"} <= set(sparse_rx.__all__)


# ---- every refusal of the call ----------------------------------------------------------------------------------------------------
def _cols(*descs):
    arr = (_capi.FieldColDesc * len(descs))()
    for i, (data, valid, typ) in enumerate(descs):
        arr[i].data, arr[i].valid, arr[i].type = data, valid, typ
    return arr


def _call(L, device=0, cols=None, n_cols=2, n_docs=1000, doc_base=0, clauses=P[4], n_clauses=2, knots=P[5], n_knots=300, score_mode=0, boost_mode=0,
          cand_doc=P[6], cand_score=P[7], cand_count=P[8], carry_doc=P[9], carry_score=P[10], carry_count=P[11], nq=3, m=100, kc=10, k=10,
          out_doc=P[12], out_score=P[13], out_count=P[14], out_pos=P[15], stream=None):
    if cols is None:
        cols = _cols((P[0], P[1], 1), (P[2], None, 2))
    return L.srx_boost_topk(device, cols, n_cols, n_docs, doc_base, clauses, n_clauses, knots, n_knots, score_mode, boost_mode, cand_doc, cand_score,
                            cand_count, carry_doc, carry_score, carry_count, nq, m, kc, k, out_doc, out_score, out_count, out_pos, stream)


def refusals():
    """Every refusal of ``srx_boost_topk``: all return SRX_ERR_INVALID with their message, none touches a device (the pointers are
    never dereferenced).  tests/test_boost_gpu.py runs the same list on the GPU machine."""
    L = _capi.lib()

    def refused(rc, word):
        msg = L.srx_last_error()
        assert rc == -1 and word.encode() in msg, (rc, msg, word)

    no_carry = dict(carry_doc=None, carry_score=None, carry_count=None, kc=0)
    refused(_call(L, cols=ctypes.cast(None, ctypes.POINTER(_capi.FieldColDesc))), "null cols")
    for n in (0, -1, 9, 33):
        refused(_call(L, n_cols=n), "n_cols must be in [1, 8]")
    refused(_call(L, cols=_cols((P[0], None, 3), (P[2], None, 2))), "SET64")
    refused(_call(L, cols=_cols((P[0], None, 0), (P[2], None, 3))), "SET64")
    for typ in (-1, 4, 99):
        refused(_call(L, cols=_cols((P[0], None, typ), (P[2], None, 2))), "unknown column type")
    for typ in (0, 1, 2):
        refused(_call(L, cols=_cols((None, None, typ), (P[2], None, 2))), "null data")
    for typ, off in ((0, 2), (0, 1), (2, 2), (1, 4), (1, 2)):
        refused(_call(L, cols=_cols((P[0], None, 0), (P[2] + off, None, typ))), "aligned for its type")
    for off in (4, 8, 2):
        refused(_call(L, cols=_cols((P[0], P[1] + off, 0), (P[2], None, 2))), "validity row must be 16-byte aligned")
    for n in (0, -3, 2 ** 31 - 1, 2 ** 40):
        refused(_call(L, n_docs=n), "n_docs must be in [1, 2^31 - 2]")
    refused(_call(L, doc_base=-1), "negative doc_base")
    for n in (0, -1, 9):
        refused(_call(L, n_clauses=n), "n_clauses must be in [1, 8]")
    for n in (1, 0, -5, (1 << 24) + 1):
        refused(_call(L, n_knots=n), "n_knots must be in [2, 2^24]")
    for mode in (-1, 4, 99):
        refused(_call(L, score_mode=mode), "unknown score_mode")
    for mode in (-1, 3, 99):
        refused(_call(L, boost_mode=mode), "unknown boost_mode")
    for m in (0, -1):
        refused(_call(L, m=m, k=1), "m must be >= 1")
    refused(_call(L, kc=-1), "kc must be >= 0")
    for m, kc in ((2049, 0), (2048, 1), (1, 2048), (2 ** 31 - 1, 2 ** 31 - 1)):
        refused(_call(L, m=m, kc=kc, k=1, **({} if kc else {"carry_doc": None, "carry_score": None, "carry_count": None})), "m + kc must not exceed 2048")
    for k in (0, -1, 111):
        refused(_call(L, k=k), "k must be in [1, m + kc]")
    refused(_call(L, nq=-1), "nq < 0")
    refused(_call(L, nq=2 ** 31 - 1, m=2048, **no_carry), "nq * (m + kc) must not exceed 2^31 - 1")
    for name in ("carry_doc", "carry_score", "carry_count"):
        refused(_call(L, **{**dict(carry_doc=None, carry_score=None, carry_count=None, kc=0), name: P[9]}), "a carry given with kc == 0")
    for name in ("clauses", "knots"):
        refused(_call(L, **{name: None}), "null clauses / knots")
    for name in ("cand_doc", "cand_score"):
        refused(_call(L, **{name: None}), "null cand_doc / cand_score")
    for name in ("carry_doc", "carry_score"):
        refused(_call(L, **{name: None}), "kc > 0 needs carry_doc and carry_score")
    for name in ("out_doc", "out_score", "out_count"):
        refused(_call(L, **{name: None}), "null out_doc / out_score / out_count")
    # nq == 0 is fine whatever the pointers are, and is no launch
    assert _call(L, nq=0, clauses=None, knots=None, cand_doc=None, cand_score=None, out_doc=None, out_score=None, out_count=None, **no_carry) == 0
    assert _call(L, nq=0) == 0


def test_entry_point_refusals():
    refusals()


# ---- the resolver -----------------------------------------------------------------------------------------------------------------
def _columns(n=50, seed=0):
    rng = np.random.default_rng(seed)
    return host_columns({"date": rng.integers(1_600_000_000, 1_700_000_000, n).astype(np.int64), "votes": rng.integers(0, 5000, n).astype(np.int32),
                         "price": (rng.random(n) * 100).astype(np.float32), "tags": [["a"] if i % 2 else ["b", "c"] for i in range(n)],
                         "src": ["x" if i % 3 else "y" for i in range(n)]})


def _decay(kind, **kw):
    return {"functions": [{"decay": {"field": "date", "origin": 1_650_000_000, "scale": 86400 * 30, "kind": kind, **kw}}]}


@pytest.mark.parametrize("kind", ["gauss", "exp", "linear"])
def test_decay_is_elasticsearchs_formula_at_the_knots(kind):
    scale, decay, offset = 86400.0 * 30, 0.5, 86400.0 * 2
    r = boost.BoostResolver(_columns(), _decay(kind, offset=offset, decay=decay))
    f = r.functions[0]
    assert f.abs and f.origin == 1_650_000_000 and len(f.knots) == 257 and r.clauses["n_seg"][0] == 256 and r.clauses["flags"][0] == 1
    x = np.arange(257, dtype=np.float64) / float(f.inv_step)  # the offsets the device's t = x * inv_step calls 0, 1, .., 256
    d = np.maximum(0.0, x - offset)
    if kind == "gauss":
        sigma2 = -scale ** 2 / (2.0 * math.log(decay))
        want = np.exp(-d ** 2 / (2.0 * sigma2))
    elif kind == "exp":
        want = np.exp(math.log(decay) / scale * d)
    else:
        s = scale / (1.0 - decay)
        want = np.maximum(0.0, (s - d) / s)
    assert np.allclose(f.knots.astype(np.float64), want, rtol=0, atol=2.0 ** -24)  # one float32 rounding of values <= 1
    assert np.all(f.knots[x <= offset] == 1.0)
    # decay at the distance scale beyond the offset; the curve ends at the tail (linear: at 0)
    assert abs(float(np.interp(offset + scale, x, f.knots.astype(np.float64))) - decay) < 1e-3
    assert abs(float(f.knots[-1]) - (0.0 if kind == "linear" else 1e-3)) < 1e-5
    assert r.names == ["date"] and r.knots.dtype == np.float32 and np.array_equal(r.knots, f.knots)


@pytest.mark.parametrize("kind", ["gauss", "exp"])
def test_max_dev_is_below_the_second_derivative_bound(kind):
    """Linear interpolation over a segment of width h errs by at most h^2 / 8 max|f''|; the float32 rounding of a knot adds at most
    2^-25 (values <= 1, to nearest).  gauss: |f''| <= 1 / sigma^2; exp: |f''| <= lambda^2 (offset 0: no kink inside a segment)."""
    scale, decay = 1000.0, 0.5
    r = boost.BoostResolver(_columns(), {"functions": [{"decay": {"field": "votes", "origin": 100, "scale": scale, "kind": kind, "decay": decay}}]})
    f = r.functions[0]
    h = 1.0 / float(f.inv_step)
    curv = -2.0 * math.log(decay) / scale ** 2 if kind == "gauss" else (math.log(decay) / scale) ** 2
    assert len(f.knots) == 257 and 0 < r.max_dev[0] <= h * h / 8.0 * curv + 2.0 ** -25
    assert r.max_dev[0] < 2e-4  # 256 segments: the table is the formula to four digits
    coarse = boost.BoostResolver(_columns(), {"functions": [{"decay": {"field": "votes", "origin": 100, "scale": scale, "kind": kind, "segments": 16}}]})
    assert coarse.max_dev[0] > 10 * r.max_dev[0]


def test_field_value_and_curve():
    cols = _columns()
    r = boost.BoostResolver(cols, {"functions": [{"field_value": {"field": "votes", "lo": 0, "hi": 5000, "modifier": "log1p", "factor": 0.5, "weight": 2,
                                                                   "missing": 0}},
                                                 {"field_value": {"field": "price", "lo": 1.5, "hi": 99.0}},
                                                 {"curve": {"field": "date", "origin": 1_600_000_000, "step": 1000, "knots": [1, 2, 0.5], "abs": False,
                                                            "weight": -1}}],
                                   "score_mode": "sum", "boost_mode": "sum"})
    a, b, c = r.functions
    x = np.arange(257, dtype=np.float64) / float(a.inv_step)
    assert np.allclose(a.knots, np.log1p(0.5 * x), atol=1e-6) and not a.abs and a.origin == 0 and float(a.weight) == 2 and float(a.missing) == 0
    # log1p bends most at 0, where a segment is 19.5 votes wide: the table is coarse there and max_dev says so (|f''| <= factor^2)
    mid = 0.5 / float(a.inv_step)
    assert abs(r.max_dev[0] - (math.log1p(0.5 * mid) - 0.5 * math.log1p(mid))) < 1e-6 and 0.5 < r.max_dev[0] < (2 * mid) ** 2 / 8 * 0.25
    assert len(b.knots) == 2 and b.origin == boost_ref.f32_bits(1.5) and r.max_dev[1] < 1e-5 and abs(float(b.knots[1]) - 99.0) < 1e-4
    assert c.knots.tolist() == [1.0, 2.0, 0.5] and float(c.inv_step) == np.float32(1e-3) and r.max_dev[2] is None and float(c.weight) == -1
    assert r.names == ["votes", "price", "date"] and r.clauses["col"].tolist() == [0, 1, 2]
    assert r.clauses["knot0"].tolist() == [0, 257, 259] and r.clauses["n_seg"].tolist() == [256, 1, 2] and len(r.knots) == 262
    assert (r.score_mode, r.boost_mode) == (1, 1)
    boost.check_clause_arrays([0, 2, 1], r.clauses, r.knots)
    for mod, fn in (("sqrt", np.sqrt), ("square", np.square), ("none", lambda z: z)):
        q = boost.BoostResolver(cols, {"functions": [{"field_value": {"field": "votes", "lo": 0, "hi": 100, "modifier": mod, "segments": 50}}]})
        assert np.allclose(q.functions[0].knots, fn(np.arange(51) * 2.0), rtol=1e-6)


@pytest.mark.parametrize("score_mode", ["multiply", "sum", "max", "min"])
def test_f_bounds_hold_over_random_columns(score_mode):
    smode = boost.SCORE_MODES[score_mode]
    for seed in range(40):
        rng = np.random.default_rng(seed)
        n = 400
        cols = host_columns({"a": rng.integers(-3000, 3000, n).astype(np.int32), "b": rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64),
                             "c": np.ma.masked_array((rng.standard_normal(n) * 50).astype(np.float32), mask=rng.random(n) < 0.2)})
        fns = []
        for j in range(int(rng.integers(1, 9))):
            field = "abc"[j % 3]
            span = {"a": 2000.0, "b": 10.0 ** 12, "c": 60.0}[field]
            n_knots = int(rng.integers(2, 40))
            fns.append({"curve": {"field": field, "origin": int(rng.integers(-100, 100)), "step": span / n_knots * float(rng.random() + 0.2),
                                  "knots": (rng.standard_normal(n_knots) * 2).tolist(), "abs": bool(rng.integers(0, 2)),
                                  "weight": float(rng.standard_normal()), "missing": float(rng.standard_normal())}})
        r = boost.BoostResolver(cols, {"functions": fns, "score_mode": score_mode})
        ref_cols = [(cols[nm].type, cols[nm].data, cols[nm].valid) for nm in r.names]
        local = np.arange(n)
        F = boost_ref.fold([boost_ref.factor(ref_cols[int(c["col"])], c, r.knots, local) for c in r.clauses], smode)
        assert r.F_lo.dtype == np.float32 and r.F_lo <= F.min() and F.max() <= r.F_hi, (seed, r.F_lo, F.min(), F.max(), r.F_hi)


def test_f_bounds_cover_a_lerp_that_rounds_past_its_knot():
    cols = host_columns({"a": np.arange(10, dtype=np.int32)})
    r = boost.BoostResolver(cols, {"functions": [{"curve": {"field": "a", "origin": 0, "step": 100, "knots": [0.1, 0.7]}}]})
    y = r.knots
    assert r.F_lo == y[0] and r.F_hi >= max(y[1], np.float32(y[0] + np.float32(y[1] - y[0])))


def test_resolver_refusals():
    cols = _columns()
    ok = {"field": "date", "origin": 1_650_000_000, "scale": 1000}
    bad_specs = [None, [], {"functions": []}, {"functions": [{"decay": ok}] * 9}, {"functions": [{"decay": ok}], "score_mode": "avg"},
                 {"functions": [{"decay": ok}], "boost_mode": "max"}, {"functions": [{"decay": ok}], "mode": "sum"}, {"functions": [{"gauss": ok}]},
                 {"functions": [{"decay": ok, "curve": ok}]}, {"functions": [{"decay": 3}]}, {"functions": ["decay"]}]
    for spec in bad_specs:
        with pytest.raises(ValueError):
            boost.BoostResolver(cols, spec)
    bad_decay = [{"field": "nope"}, {"field": "tags"}, {"scale": 0}, {"scale": -1}, {"scale": float("inf")}, {"scale": "1"}, {"offset": -1}, {"decay": 0},
                 {"decay": 1}, {"tail": 0}, {"tail": 1}, {"kind": "cauchy"}, {"segments": 0}, {"segments": 2.5}, {"segments": 1 << 24}, {"origin": 0.5},
                 {"origin": 2 ** 63}, {"origin": None}, {"weight": float("nan")}, {"weight": 1e39}, {"missing": float("inf")}, {"extra": 1}]
    for kw in bad_decay:
        with pytest.raises(ValueError):
            boost.BoostResolver(cols, {"functions": [{"decay": {**ok, **kw}}]})
    for drop in ("origin", "scale", "field"):
        with pytest.raises(ValueError):
            boost.BoostResolver(cols, {"functions": [{"decay": {k: v for k, v in ok.items() if k != drop}}]})
    fv = {"field": "votes", "lo": 0, "hi": 10}
    for kw in ({"hi": 0}, {"hi": -1}, {"modifier": "ln"}, {"modifier": "log1p", "lo": -5}, {"modifier": "sqrt", "lo": -5}, {"factor": float("nan")},
               {"lo": 0.5}, {"field": "tags"}, {"segments": -1}):
        with pytest.raises(ValueError):
            boost.BoostResolver(cols, {"functions": [{"field_value": {**fv, **kw}}]})
    cv = {"field": "price", "origin": 0.0, "step": 1.0, "knots": [1, 2]}
    for kw in ({"knots": [1]}, {"knots": []}, {"knots": "12"}, {"knots": [1, float("nan")]}, {"knots": [1, 1e39]}, {"step": 0}, {"step": -2}, {"step": 1e-46},
               {"step": float("inf")}, {"abs": 1}, {"origin": float("nan")}, {"field": "tags"}):
        with pytest.raises(ValueError):
            boost.BoostResolver(cols, {"functions": [{"curve": {**cv, **kw}}]})
    with pytest.raises(ValueError, match="overflows float32"):
        boost.BoostResolver(cols, {"functions": [{"curve": {**cv, "knots": [1e30, 2e30], "weight": 1e30}}]})
    # a category column is its code: a number, allowed
    assert boost.BoostResolver(cols, {"functions": [{"curve": {"field": "src", "origin": 0, "step": 1, "knots": [1, 2]}}]}).names == ["src"]


def test_check_clause_arrays():
    r = boost.BoostResolver(_columns(), {"functions": [{"curve": {"field": "votes", "origin": 0, "step": 1, "knots": [1, 2, 3]}}]})
    boost.check_clause_arrays([0], r.clauses, r.knots)
    for field, value in (("col", 1), ("col", -1), ("n_seg", 0), ("n_seg", 3), ("knot0", -1), ("knot0", 1), ("inv_step", 0.0), ("inv_step", -1.0),
                         ("inv_step", np.inf), ("inv_step", np.nan), ("weight", np.nan), ("missing", np.inf)):
        c = r.clauses.copy()
        c[field][0] = value
        with pytest.raises(ValueError):
            boost.check_clause_arrays([0], c, r.knots)
    with pytest.raises(ValueError):
        boost.check_clause_arrays([3], r.clauses, r.knots)
    with pytest.raises(ValueError):
        boost.check_clause_arrays([0], r.clauses, np.array([1, np.inf, 2], dtype=np.float32))
    with pytest.raises(ValueError):
        boost.check_clause_arrays([0], r.clauses.view(np.uint8), r.knots)


# ---- boost_deep over a fake search ------------------------------------------------------------------------------------------------
class _FakeSearch:
    """Rankings on CPU tensors: query q's complete ranking is ``rankings[q]`` = (docs, scores) in the engine's order (score
    descending, doc id ascending), scores > 0.  A call returns the next kk rows ranked strictly after the bound row; a bound of
    score 0 has nothing after it."""

    def __init__(self, rankings):
        self.rankings, self.calls, self.rows = rankings, [], 0

    def __call__(self, q_ptr, q_term, q_weight, kk, after=None):
        self.calls.append((int(kk), after is not None))
        nq = len(self.rankings)
        d, s, c = torch.full((nq, kk), -1, dtype=torch.int32), torch.zeros((nq, kk), dtype=torch.float32), torch.zeros(nq, dtype=torch.int32)
        for q, (docs, scores) in enumerate(self.rankings):
            start = 0
            if after is not None:
                assert after[0].dtype == torch.int32 and after[1].dtype == torch.float32
                a_doc, a_score = int(after[0][q]), np.float32(after[1][q])
                behind = (scores < a_score) | ((scores == a_score) & (docs > a_doc))
                start = int(np.argmax(behind)) if behind.any() else len(docs)
                assert a_score == 0 or (start > 0 and int(docs[start - 1]) == a_doc)  # the bound is a row of the ranking
            n = min(kk, len(docs) - start)
            d[q, :n], s[q, :n], c[q] = torch.from_numpy(docs[start: start + n]), torch.from_numpy(scores[start: start + n]), n
            self.rows += n
        return d, s, c


class _RefBoostFn:
    """``boost_fn`` of boost_deep computed by tests/boost_ref.py on CPU tensors"""

    def __init__(self, cols, n_docs, res):
        self.cols, self.n_docs, self.res = cols, n_docs, res
        self.boost_mode, self.F_lo, self.F_hi = res.boost_mode_name, res.F_lo, res.F_hi
        self.widths = []

    def __call__(self, d, s, c, kk, carry=None):
        cr = (None, None, None) if carry is None else tuple(None if t is None else t.numpy() for t in carry)
        self.widths.append((int(d.shape[1]), 0 if carry is None else int(carry[0].shape[1])))
        r = self.res
        od, ob, oc, _ = boost_ref.boost_topk(self.cols, self.n_docs, 0, list(r.clauses), r.knots, r.score_mode, r.boost_mode, d.numpy(), s.numpy(),
                                             None if c is None else c.numpy(), kk, *cr)
        return torch.from_numpy(od), torch.from_numpy(ob.view(np.float32)), torch.from_numpy(oc)


def _brute(cols, n_docs, res, rankings, k):
    """All docs scoring > 0, boosted by the restatement, the first k"""
    out = []
    for docs, scores in rankings:
        assert (scores > 0).all()
        kk = min(k, len(docs))
        d, b, c, _ = boost_ref.boost_topk(cols, n_docs, 0, list(res.clauses), res.knots, res.score_mode, res.boost_mode, docs[None], scores[None], None, kk)
        out.append((d[0, : c[0]], b[0, : c[0]]))
    return out


def _same(got, want, k):
    kd, ks, kc = (t.numpy() for t in got)
    assert kd.shape == ks.shape == (len(want), k)
    for q, (d, b) in enumerate(want):
        assert int(kc[q]) == len(d) and np.array_equal(kd[q, : len(d)], d) and np.array_equal(ks[q, : len(d)].view(np.uint32), b), q
        assert (kd[q, len(d):] == -1).all() and (ks[q, len(d):].view(np.uint32) == 0).all()


def _deep_case(seed=3, n=700, mode="multiply"):
    rng = np.random.default_rng(seed)
    date = rng.integers(0, 10_000, n).astype(np.int64)
    votes = rng.integers(0, 500, n).astype(np.int32)
    cols = host_columns({"date": date, "votes": votes})
    spec = {"functions": [{"decay": {"field": "date", "origin": 9_000, "scale": 400, "kind": "gauss", "segments": 64}},
                          {"field_value": {"field": "votes", "lo": 0, "hi": 500, "modifier": "log1p", "factor": 0.1, "segments": 32, "weight": 0.5}}],
            "score_mode": "sum", "boost_mode": mode}
    res = boost.BoostResolver(cols, spec)
    ref_cols = [(cols[nm].type, cols[nm].data, cols[nm].valid) for nm in res.names]
    rankings = []
    for length in (n, 300, 5, 37):  # the complete ranking, shorter ones, one shorter than k
        docs = rng.permutation(n)[:length].astype(np.int32)
        scores = np.round(rng.random(length) * 6 + 0.5, 1).astype(np.float32)  # one decimal: many raw ties
        order = np.lexsort((docs, -scores))
        rankings.append((docs[order], scores[order]))
    return n, ref_cols, res, rankings


@pytest.mark.parametrize("page", [4, 8, 1024])
@pytest.mark.parametrize("mode", ["multiply", "sum"])
def test_boost_deep_is_the_brute_force(page, mode):
    n, cols, res, rankings = _deep_case(mode=mode)
    for k in (1, 10):
        search, fn = _FakeSearch(rankings), _RefBoostFn(cols, n, res)
        got = boost_deep(search, fn, None, None, None, k, first=min(max(page, k), n), page=page)
        _same(got, _brute(cols, n, res, rankings, k), k)
        assert all(m + kc <= 2048 for m, kc in fn.widths) and fn.widths[0][1] == 0 and all(kc == k for _, kc in fn.widths[1:])
        if page == 4:
            assert len(search.calls) > 3  # it paged: the gauss decay moves docs far up
        if page == 1024:
            assert search.calls == [(700, False)]  # the whole ranking was page one: every query came back short or settled
    # a short first page ends a query at once: the rankings of 5 and 37 rows never see a second page of their own
    search, fn = _FakeSearch(rankings[2:]), _RefBoostFn(cols, n, res)
    got = boost_deep(search, fn, None, None, None, 10, first=64, page=8)
    assert search.calls == [(64, False)]
    _same(got, _brute(cols, n, res, rankings[2:], 10), 10)


def test_boost_deep_reads_on_when_the_bound_ties():
    """bound == k-th boosted score, and the next page holds a doc with a LOWER id that reaches the same score: a door that stops on
    equality returns doc 60, the exact one doc 7."""
    n = 100
    factor = np.ones(n, dtype=np.int32)
    factor[7] = 2
    cols = host_columns({"f": factor})
    res = boost.BoostResolver(cols, {"functions": [{"field_value": {"field": "f", "lo": 0, "hi": 2}}]})
    assert float(res.F_hi) == 2.0 and float(res.F_lo) == 0.0
    ref_cols = [(cols["f"].type, cols["f"].data, None)]
    ranking = (np.array([60, 5, 7, 9], dtype=np.int32), np.array([4.0, 2.0, 2.0, 1.0], dtype=np.float32))
    search, fn = _FakeSearch([ranking]), _RefBoostFn(ref_cols, n, res)
    kd, ks, kc = boost_deep(search, fn, None, None, None, 1, first=2, page=2)
    assert search.calls == [(2, False), (2, True)] and kc.tolist() == [1]
    assert kd.tolist() == [[7]] and ks.tolist() == [[4.0]]
    _same((kd, ks, kc), _brute(ref_cols, n, res, [ranking], 1), 1)
    # one step clear of the tie it stops after page one: bound = 1.5 * 2 = 3 < 4
    ranking = (np.array([60, 5, 7, 9], dtype=np.int32), np.array([4.0, 1.5, 1.5, 1.0], dtype=np.float32))
    search = _FakeSearch([ranking])
    kd, _, _ = boost_deep(search, _RefBoostFn(ref_cols, n, res), None, None, None, 1, first=2, page=2)
    assert search.calls == [(2, False)] and kd.tolist() == [[60]]


def test_boost_deep_max_depth_and_refusals():
    n, cols, res, rankings = _deep_case()
    search, fn = _FakeSearch(rankings[:1]), _RefBoostFn(cols, n, res)
    got = boost_deep(search, fn, None, None, None, 10, first=8, page=8, max_depth=20)
    assert search.calls == [(8, False), (8, True), (4, True)] and search.rows == 20
    docs, scores = rankings[0]
    _same(got, _brute(cols, n, res, [(docs[:20], scores[:20])], 10), 10)  # the boosted top of the rows read
    got = boost_deep(_FakeSearch(rankings[:1]), _RefBoostFn(cols, n, res), None, None, None, 10, first=64, page=8, max_depth=5)
    _same(got, _brute(cols, n, res, [(docs[:5], scores[:5])], 10), 10)
    # no bound exists: REPLACE, and a factor that can be negative under MULTIPLY
    rep = boost.BoostResolver(host_columns({"f": np.arange(5, dtype=np.int32)}), {"functions": [{"field_value": {"field": "f", "lo": 0, "hi": 4}}],
                                                                                   "boost_mode": "replace"})
    with pytest.raises(ValueError, match="replace"):
        boost_deep(_FakeSearch(rankings[:1]), _RefBoostFn(cols, n, rep), None, None, None, 3, first=8)
    neg = boost.BoostResolver(host_columns({"f": np.arange(5, dtype=np.int32)}), {"functions": [{"field_value": {"field": "f", "lo": 0, "hi": 4, "weight": -1}}]})
    assert neg.F_lo < 0
    with pytest.raises(ValueError, match="negative"):
        boost_deep(_FakeSearch(rankings[:1]), _RefBoostFn(cols, n, neg), None, None, None, 3, first=8)
    neg_sum = boost.BoostResolver(host_columns({"f": np.arange(5, dtype=np.int32)}),
                                  {"functions": [{"field_value": {"field": "f", "lo": 0, "hi": 4, "weight": -1}}], "boost_mode": "sum"})
    boost_deep(_FakeSearch(rankings[:1]), _RefBoostFn(cols, n, neg_sum), None, None, None, 3, first=8)  # SUM bounds any sign


# ---- the doors' refusals (no device is reached) -----------------------------------------------------------------------------------
def test_door_refusals():
    be = SparseBackend.__new__(SparseBackend)
    be._fields, be.host, be.dev, be.group, be._field_table = None, None, None, None, None
    be.sharded = lambda: False
    spec = {"functions": [{"decay": {"field": "date", "origin": 100, "scale": 10}}]}
    assert be.boost_spec(None) is None
    with pytest.raises(ValueError, match="set_doc_fields"):
        be.boost_spec(spec, call="search_bm25")
    be._fields = host_columns({"date": np.arange(30, dtype=np.int64), "tags": [["a"]] * 30})
    r = be.boost_spec(spec, 50, 10, "search_bm25")
    assert isinstance(r, boost.BoostResolver) and r.depth == 50 and be.boost_spec(spec).depth is None
    with pytest.raises(ValueError, match="at most 1024"):
        be.boost_spec(spec, None, 1025)
    with pytest.raises(ValueError, match="boost_depth"):
        be.boost_spec(spec, 0)
    with pytest.raises(ValueError, match="collapse"):
        be.boost_spec(spec, None, 10, "search", collapse=object())
    with pytest.raises(ValueError, match="set column"):
        be.boost_spec({"functions": [{"decay": {"field": "tags", "origin": 1, "scale": 1}}]})
    with pytest.raises(ValueError, match="unknown field"):
        be.boost_spec({"functions": [{"decay": {"field": "nope", "origin": 1, "scale": 1}}]})
    with pytest.raises(ValueError, match="replace"):
        be.boost_spec({**spec, "boost_mode": "replace"})
    assert be.boost_spec({**spec, "boost_mode": "replace"}, exact=False).boost_mode_name == "replace"
    with pytest.raises(ValueError, match="must not be negative"):
        be.boost_spec({"functions": [{"decay": {"field": "date", "origin": 1, "scale": 1, "weight": -2}}]})
    be.sharded = lambda: True
    with pytest.raises(ValueError, match="one GPU"):
        be.boost_spec(spec)
    # the keywords exist on the doors the issue names, with defaults that change nothing, and not on the others
    for fn in (sparse_rx.RetrievalService.search_bm25, sparse_rx.OptimizedBM25Retriever.search, sparse_rx.OptimizedRetriever.search):
        p = inspect.signature(fn).parameters
        assert p["boost"].default is None and p["boost_depth"].default is None
    p = inspect.signature(sparse_rx.RetrievalService.search_hybrid).parameters
    assert p["boost"].default is None and p["boost_pool"].default is None
    for cls in (sparse_rx.RetrievalService, sparse_rx.OptimizedBM25Retriever, sparse_rx.OptimizedRetriever):
        assert "top_k" in inspect.signature(cls.boost_results).parameters
    for fn in (sparse_rx.HybridRetriever.search, sparse_rx.ShardedSearcher.search, sparse_rx.HostBatchPipeline.search):
        assert "boost" not in inspect.signature(fn).parameters


# ---- the bit tests' data is sensitive to contraction ------------------------------------------------------------------------------
def test_gpu_bit_data_tells_a_fused_lerp_apart():
    """The GPU bit tests compare score bits with the restatement.  They can only pin "every operation rounded on its own" if their
    fixed-seed inputs give other bits under a fused multiply-add; here the same inputs are recomputed with the lerp's y0 + fr * dy
    as one float64 multiply-add rounded once."""
    cols = boost_ref.table()
    differing = 0
    for seed in (1, 2, 3):
        clauses, knots, d, s, c, carry = boost_ref.bit_case(seed)
        plain = boost_ref.boost_topk(cols, boost_ref.N_DOCS, boost_ref.DOC_BASE, clauses, knots, 0, 0, d, s, c, d.shape[1], *carry)
        fused = boost_ref.boost_topk(cols, boost_ref.N_DOCS, boost_ref.DOC_BASE, clauses, knots, 0, 0, d, s, c, d.shape[1], *carry, fused=True)
        assert np.array_equal(plain[2], fused[2])
        differing += int((plain[1] != fused[1]).sum())
    assert differing >= 1
