"""Learned reranking on the GPU (include/ltr/sparse_rx_ltr.h).  Expected rows are never the engine's own: the restatement
(tests/ltr_ref.py) on the columns, features, model and lists a call was given.  Every comparison is exact -- doc ids, positions,
counts and the BITS of the scores --, and every output buffer is pre-filled with 0x7f bytes so that a word the kernel does not
write shows.  3 000 docs, doc_base 1 000, 33 queries."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ltr_ref  # noqa: E402
from ltr_ref import F32, F_COLUMN, F_EXTRA, F_RANK, F_SCORE, I32, I64, LE, LT, MISSING_LEFT, NODE_DTYPE, REPLACE, SUM  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
GARBAGE = 0x7F7F7F7F
N_DOCS, DOC_BASE, NQ = 3000, 1000, 33
NAN = np.float32(np.nan)
FEATS = [(F_SCORE, 0), (F_RANK, 0), (F_COLUMN, 0), (F_COLUMN, 1), (F_COLUMN, 2), (F_EXTRA, 0), (F_EXTRA, 2), (F_COLUMN, 3)]  # every kind
N_EXTRA = 3


def table():
    """[(type, data, valid)]: an I32 column with a validity row, an I64 column whose first rows hold the conversion's edges, an F32
    column with NaNs, zeros of both signs and infinities (and a validity row), a plain I64 column"""
    rng = np.random.default_rng(11)
    votes = rng.integers(-50, 50, N_DOCS).astype(np.int32)
    votes[:4] = [(1 << 24) + 1, -(1 << 24) - 1, 2 ** 31 - 1, -2 ** 31]
    big = rng.integers(-10 ** 12, 10 ** 12, N_DOCS).astype(np.int64)
    big[:10] = [(1 << 24) + 1, (1 << 24) + 3, (1 << 24) + 2, 2 ** 63 - 1, 2 ** 63 - 2 ** 38 - 1, 2 ** 63 - 2 ** 38, -2 ** 63, (1 << 53) + 1, -(1 << 24) - 1, 0]
    price = (rng.standard_normal(N_DOCS) * 20).astype(np.float32)
    price[:8] = [NAN, 0.0, -0.0, np.inf, -np.inf, 1.5, np.float32(1.5) + np.float32(2.0 ** -23), 3.4e38]
    price[rng.random(N_DOCS) < 0.05] = NAN
    small = rng.integers(0, 8, N_DOCS).astype(np.int64)  # few distinct values: thresholds on them tie often
    has_votes = rng.random(N_DOCS) > 0.2
    has_votes[:4] = True
    return [(I32, votes, has_votes), (I64, big, None), (F32, price, np.arange(N_DOCS) % 11 != 5), (I64, small, None)]


class _Table:
    """The columns on the device, as the C calls take them, next to their host arrays"""

    def __init__(self, cols, n_docs=N_DOCS, doc_base=DOC_BASE):
        import torch
        from sparse_rx import _capi
        from sparse_rx.filter import pack_masks
        self.cols, self.n_docs, self.doc_base = cols, n_docs, doc_base
        self.keep = []
        self.desc = (_capi.FieldColDesc * max(len(cols), 1))()
        for i, (typ, data, valid) in enumerate(cols):
            d_t = torch.from_numpy(np.ascontiguousarray(data)).to(DEVICE)
            v_t = None if valid is None else torch.from_numpy(pack_masks(np.asarray(valid, dtype=bool)).view(np.int32).copy()).to(DEVICE).reshape(-1)
            self.keep += [d_t, v_t]
            self.desc[i].data, self.desc[i].valid, self.desc[i].type = d_t.data_ptr(), None if v_t is None else v_t.data_ptr(), typ

    def _head(self, feats, extra, model, mode, doc, score, count):
        import torch
        from sparse_rx import _capi
        up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEVICE)
        nodes, tree_ptr, base, cmp = model
        far = (_capi.LtrFeature * len(feats))()
        for i, (kind, index) in enumerate(feats):
            far[i].kind, far[i].index = kind, index
        t = dict(doc=up(doc, np.int32), score=up(score, np.float32), count=up(count, np.int32), extra=up(extra, np.float32),
                 nodes=torch.from_numpy(np.ascontiguousarray(nodes).view(np.uint8).copy()).to(DEVICE), tree_ptr=up(tree_ptr, np.int32))
        ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
        nq, m = doc.shape
        n_cols = len(self.cols)
        head = (0, self.desc if n_cols else None, n_cols, self.n_docs, self.doc_base, far, len(feats), ptr(t["extra"]), 0 if extra is None else extra.shape[2],
                ptr(t["nodes"]), len(nodes), ptr(t["tree_ptr"]), len(tree_ptr) - 1, float(base), cmp, mode, ptr(t["doc"]), ptr(t["score"]), ptr(t["count"]), nq, m)
        return head, t, far

    def run_topk(self, feats, extra, model, mode, doc, score, count, k, pos=True, stream=None, twice=False):
        """srx_ltr_topk on garbage-filled outputs -> host (doc, score bits, count, pos | None)"""
        import torch
        from sparse_rx import _capi
        head, keep, far = self._head(feats, extra, model, mode, doc, score, count)
        nq = doc.shape[0]
        o_doc, o_score, o_pos = (torch.full((nq, k), GARBAGE, dtype=torch.int32, device=DEVICE) for _ in range(3))
        o_count = torch.full((nq,), GARBAGE, dtype=torch.int32, device=DEVICE)
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        for _ in range(2 if twice else 1):
            rc = _capi.lib().srx_ltr_topk(*head, k, o_doc.data_ptr(), o_score.data_ptr(), o_count.data_ptr(), o_pos.data_ptr() if pos else None, sp)
            _capi.check(rc, "srx_ltr_topk")
        torch.cuda.synchronize()
        return (o_doc.cpu().numpy(), o_score.cpu().numpy().view(np.uint32), o_count.cpu().numpy(), o_pos.cpu().numpy() if pos else None)

    def run_score(self, feats, extra, model, mode, doc, score, count, stream=None):
        """srx_ltr_score on a garbage-filled output -> host bits [nq, m]"""
        import torch
        from sparse_rx import _capi
        head, keep, far = self._head(feats, extra, model, mode, doc, score, count)
        out = torch.full(doc.shape, GARBAGE, dtype=torch.int32, device=DEVICE)
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        _capi.check(_capi.lib().srx_ltr_score(*head, out.data_ptr(), sp), "srx_ltr_score")
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)

    def reference(self, feats, extra, model, mode, doc, score, count):
        nodes, tree_ptr, base, cmp = model
        return ltr_ref.new_scores(self.cols, self.n_docs, self.doc_base, feats, extra, nodes, tree_ptr, base, cmp, mode, doc, score, count)

    def check(self, feats, extra, model, mode, doc, score, count, ks, what=None, **kw):
        """Both entry points against the restatement, whose scores are computed once for every k of ``ks``"""
        live, bits = self.reference(feats, extra, model, mode, doc, score, count)
        got = self.run_score(feats, extra, model, mode, doc, score, count)
        assert np.array_equal(got, bits), (what, "srx_ltr_score", np.argwhere(got != bits)[:5].tolist())
        for k in ks:
            got = self.run_topk(feats, extra, model, mode, doc, score, count, k, **kw)
            want = ltr_ref.select(live, bits, doc, k)
            for g, w, name in zip(got, want, ("doc", "score bits", "count", "pos")):
                assert g is None or np.array_equal(g, w), (what, k, name, np.argwhere(g != w)[:5].tolist())
        return live, bits


@pytest.fixture(scope="module")
def tab():
    return _Table(table())


# ---- models and lists ------------------------------------------------------------------------------------------------------------------
def forest(rng, n_trees, depth, n_features, thresholds, leaf=None, p_leaf=0.15):
    """Random trees in pre-order (every child ahead of its node): (nodes, tree_ptr).  ``thresholds``: feature -> the values a split
    draws from; ``leaf``: rng -> a leaf value (default: magnitudes from 1e-4 to 1e7, either sign, so that the sum's order shows)"""
    leaf = leaf or (lambda r: np.float32(r.standard_normal() * 10.0 ** r.integers(-4, 8)))
    recs, ptr = [], [0]
    for _ in range(n_trees):
        tree = []

        def grow(d):
            i = len(tree)
            if d == depth or (d > 0 and rng.random() < p_leaf):
                tree.append((-1, leaf(rng), 0, 0))
                return i
            f = int(rng.integers(0, n_features))
            tree.append(None)
            l = grow(d + 1)
            r = grow(d + 1)
            tree[i] = (f | (MISSING_LEFT if rng.random() < 0.5 else 0), np.float32(rng.choice(thresholds[f])), l - 0, r - 0)
            return i

        grow(0)
        recs += tree
        ptr.append(len(recs))
    return np.array(recs, dtype=NODE_DTYPE), np.array(ptr, dtype=np.int32)


def thresholds_of(cols, feats, m):
    """feature -> candidate thresholds, many of them values the feature takes (so that x == threshold happens)"""
    out = []
    for kind, index in feats:
        if kind == F_COLUMN:
            data = cols[index][1]
            out.append(np.concatenate([data[:16].astype(np.float32), data[::97].astype(np.float32)]))
        elif kind == F_RANK:
            out.append(np.arange(0, max(m, 2), max(1, m // 7), dtype=np.float32))
        else:
            out.append(np.float32([-1.0, -0.25, 0.0, 0.25, 0.5, 1.0, 2.0]))
    return [t[~np.isnan(t)] for t in out]


def lists(seed, nq, m, counts=True):
    """Candidate lists: distinct doc ids per query, some outside [doc_base, doc_base + n_docs); scores in quarter steps (they tie
    with thresholds and with each other) with NaN, infinities and zeros of both signs; counts on and past every edge; an extra plane
    with NaNs"""
    rng = np.random.default_rng(seed)
    doc = np.stack([rng.choice(np.arange(DOC_BASE - 60, DOC_BASE + N_DOCS + 60), size=m, replace=False) for _ in range(nq)]).astype(np.int32) \
        if nq else np.zeros((0, m), np.int32)
    score = (rng.integers(-8, 9, (nq, m)) / 4.0).astype(np.float32)
    special = rng.random((nq, m))
    for lo, v in ((0.00, NAN), (0.02, np.inf), (0.03, -np.inf), (0.04, -0.0)):
        score[(special >= lo) & (special < lo + 0.01 + 0.01 * (lo == 0))] = v
    count = None
    if counts:
        count = rng.integers(0, m + 1, nq).astype(np.int32)
        count[:6] = [0, -3, m + 5, m, 1, max(m - 1, 0)][: min(6, nq)]
    extra = (rng.integers(-8, 9, (nq, m, N_EXTRA)) / 4.0).astype(np.float32)
    extra[rng.random(extra.shape) < 0.1] = NAN
    return doc, score, count, extra


# ---- 1. geometry: the tile edges, k = 1 and k = m, both modes, both entry points --------------------------------------------------
@pytest.mark.parametrize("m", [1, 40, 255, 256, 257, 2048])
def test_tile_edges(tab, m):
    rng = np.random.default_rng(100 + m)
    n_trees, depth = (3, 3) if m == 2048 else (7, 4)
    nodes, ptr = forest(rng, n_trees, depth, len(FEATS), thresholds_of(tab.cols, FEATS, m))
    doc, score, count, extra = lists(200 + m, NQ, m)
    mode = REPLACE if m % 2 else SUM
    tab.check(FEATS, extra, (nodes, ptr, np.float32(0.375), LE), mode, doc, score, count, sorted({1, m}), what=m)
    if m <= 257:  # a NULL count: every position counts; the other mode, the other compare
        tab.check(FEATS, extra, (nodes, ptr, np.float32(-2.5), LT), SUM if mode == REPLACE else REPLACE, doc, score, None, sorted({1, m}), what=(m, "null count"))


@pytest.mark.parametrize("nq", [0, 1, 300])
def test_query_counts(tab, nq):
    rng = np.random.default_rng(7)
    nodes, ptr = forest(rng, 2, 2, len(FEATS), thresholds_of(tab.cols, FEATS, 9))
    doc, score, count, extra = lists(300 + nq, nq, 9)
    tab.check(FEATS, extra, (nodes, ptr, np.float32(1.0), LE), REPLACE, doc, score, count, [1, 9], what=nq)


def test_counts_and_docs_outside_the_index(tab):
    m = 40
    rng = np.random.default_rng(8)
    nodes, ptr = forest(rng, 5, 3, len(FEATS), thresholds_of(tab.cols, FEATS, m))
    doc, score, _, extra = lists(9, NQ, m)
    count = np.array(([0, -1, -2 ** 31, m + 1, 2 ** 31 - 1, m, m - 1, 1] * 5)[:NQ], np.int32)
    doc[7] = np.arange(m) + DOC_BASE + N_DOCS  # every doc past the table: an empty result
    doc[6, ::2] = DOC_BASE - 1 - np.arange(m // 2)  # every other one before it
    doc[5, :4] = [DOC_BASE, DOC_BASE + N_DOCS - 1, 2 ** 31 - 1, -2 ** 31]  # the edges of the table and of int32
    live, _ = tab.check(FEATS, extra, (nodes, ptr, np.float32(0.0), LE), REPLACE, doc, score, count, [1, 17, m])
    assert not live[0].any() and not live[1].any() and not live[7].any() and live[5, :2].all() and not live[5, 2:4].any() and not live[6, ::2].any() and live[6, 1::2].any()


# ---- 2. the features: every kind, the conversions, missing values under both directions, the compares' edges ------------------------
def stumps(feats_thresholds, cmp_leaf_seed=0):
    """One stump per (feature, threshold, missing-goes-left): x cmp thr ? a : b with distinct leaves"""
    rng = np.random.default_rng(cmp_leaf_seed)
    recs = []
    for f, thr in feats_thresholds:
        for left in (0, MISSING_LEFT):
            recs += [(f | left, np.float32(thr), 1, 2), (-1, np.float32(rng.integers(1, 2 ** 20)), 0, 0), (-1, np.float32(-rng.integers(1, 2 ** 20)) / 8, 0, 0)]
    return np.array(recs, dtype=NODE_DTYPE), np.arange(0, len(recs) + 1, 3, dtype=np.int32)


@pytest.mark.parametrize("cmp", [LE, LT])
def test_value_edges(tab, cmp):
    """The first rows of the table hold the edges: an I64 above 2^24 (2^24 + 1 and + 3 round to different evens), near 2^63, an I32
    above 2^24, an F32 NaN, zeros of both signs, infinities, a cleared valid bit.  One stump per threshold and default direction, the
    thresholds the converted values themselves and their neighbours, +0 / -0, the infinities and a NaN."""
    f32 = np.float32
    edges = {2: [f32(1 << 24), f32((1 << 24) + 2), f32(2 ** 31), f32(-2 ** 31), f32(3.0)],  # feature 2: the I32 column
             3: [f32(1 << 24), f32((1 << 24) + 2), f32((1 << 24) + 4), f32(2 ** 63), np.nextafter(f32(2 ** 63), f32(0)), f32(-2 ** 63), f32(2 ** 53), f32(0.0)],
             4: [f32(0.0), f32(-0.0), f32(np.inf), f32(-np.inf), NAN, f32(1.5), np.nextafter(f32(1.5), f32(2)), f32(3.4e38)],  # the F32 column
             0: [f32(0.0), f32(-0.0), f32(0.25), f32(np.inf), f32(-np.inf), NAN], 1: [f32(0.0), f32(1.0), f32(15.0), f32(16.0)],
             5: [f32(0.25), f32(-0.0), NAN], 6: [f32(-2.0), f32(2.0)], 7: [f32(3.0), f32(7.0), f32(-1.0)]}
    nodes, ptr = stumps([(f, t) for f, ts in edges.items() for t in ts], cmp)
    m = 32
    doc = np.stack([np.arange(m) + DOC_BASE, np.arange(m)[::-1] + DOC_BASE, np.arange(m) * 11 + DOC_BASE + 5]).astype(np.int32)
    _, score, _, extra = lists(12, 3, m)
    score[0, :6] = [0.0, -0.0, 0.25, np.inf, -np.inf, NAN]
    extra[0, :4, 0] = [0.25, -0.0, 0.0, NAN]
    for mode in (REPLACE, SUM):
        live, bits = tab.check(FEATS, extra, (nodes, ptr, np.float32(0.5), cmp), mode, doc, score, None, [m], what=(cmp, mode))
    assert live.all()
    # the planted rows went where the contract says: 2^24 + 1 -> 2^24 (left of "<= 2^24"), 2^24 + 3 -> 2^24 + 4 (right of "<= 2^24 + 2")
    x = lambda local, f: ltr_ref.feature_value(*FEATS[f], tab.cols, local, 0.0, 0, extra[0, 0])
    assert x(0, 3) == f32(1 << 24) and x(1, 3) == f32((1 << 24) + 4) and x(2, 3) == f32((1 << 24) + 2) and x(3, 3) == f32(2 ** 63)
    assert x(4, 3) == np.nextafter(f32(2 ** 63), f32(0)) and x(5, 3) == f32(2 ** 63) and x(7, 3) == f32(2 ** 53) and x(0, 2) == f32(1 << 24)
    assert np.isnan(x(0, 4)) and np.isnan(x(5, 4)) and not tab.cols[2][2][5]  # an F32 NaN, and a cleared bit over a number


# ---- 3. tree shapes -------------------------------------------------------------------------------------------------------------------
def test_root_leaf_one_tree_and_a_chain(tab):
    m = 40
    doc, score, count, extra = lists(13, NQ, m)
    leaf_only = (np.array([(-1, 2.5, 0, 0)], dtype=NODE_DTYPE), np.array([0, 1], np.int32), np.float32(-1.0), LE)
    tab.check(FEATS, extra, leaf_only, SUM, doc, score, count, [1, m], what="root leaf")
    # every new score equal: the doc id alone decides, and out_pos is optional
    tab.check(FEATS, extra, leaf_only, REPLACE, doc, score, None, [m], what="ties", pos=False)
    rng = np.random.default_rng(14)
    one = forest(rng, 1, 5, len(FEATS), thresholds_of(tab.cols, FEATS, m), p_leaf=0.0)
    tab.check(FEATS, extra, (*one, np.float32(0.0), LT), REPLACE, doc, score, count, [1, m], what="T = 1")
    # a chain 40 splits deep on the rank: "rank <= d" leaves at depth d, so position c walks min(c, 40) + 1 nodes
    recs = []
    for d in range(40):
        recs += [(1, np.float32(d), 2 * d + 1, 2 * d + 2), (-1, np.float32(100 - d), 0, 0)]  # node 2 d: left = the leaf 2 d + 1, right = node 2 d + 2
    recs.append((-1, np.float32(-7.0), 0, 0))
    chain = np.array(recs, dtype=NODE_DTYPE)
    live, bits = tab.check(FEATS, extra, (chain, np.array([0, 81], np.int32), np.float32(0.0), LE), REPLACE, doc, score, None, [1, m], what="chain")
    alive = np.flatnonzero(live[2])
    assert all(bits[2, c].view(np.float32) == np.float32(100 - c) for c in alive)


def test_three_hundred_trees_and_the_order_of_the_sum(tab):
    m = 20
    rng = np.random.default_rng(15)
    feats = FEATS[:5]
    big_small = lambda r: np.float32([16777216.0, -16777216.0, 3.0, 0.37, -0.73, 1.0, 1e8, -1e8][int(r.integers(0, 6 + 2 * (r.random() < 0.05)))])  # a + b + c depends on the order
    nodes, ptr = forest(rng, 300, 2, len(feats), thresholds_of(tab.cols, feats, m), leaf=big_small)
    doc, score, count, _ = lists(16, NQ, m)
    live, bits = tab.check(feats, None, (nodes, ptr, np.float32(0.1), LE), REPLACE, doc, score, count, [1, m])
    # the data can tell: adding the same contributions in the reverse tree order gives other bits for some candidates
    differ = 0
    for q, c in np.argwhere(live)[:40]:
        x = [ltr_ref.feature_value(k, i, tab.cols, int(doc[q, c]) - DOC_BASE, score[q, c], c, None) for k, i in feats]
        outs = [ltr_ref.tree_output(nodes, int(ptr[t]), int(ptr[t + 1]), len(nodes), len(feats), LE, x) for t in range(300)]
        fwd = back = np.float32(0.1)
        for a, b in zip(outs, outs[::-1]):
            fwd, back = np.float32(fwd + a), np.float32(back + b)
        assert ltr_ref.f32_bits(fwd) == int(bits[q, c])
        differ += int(ltr_ref.f32_bits(fwd) != ltr_ref.f32_bits(back))
    assert differ > 0


# ---- 4. malformed models: the defined +0 outcomes -----------------------------------------------------------------------------------
def test_malformed_models_contribute_zero(tab):
    m = 40
    doc, score, count, extra = lists(17, NQ, m)
    L, R = (-1, np.float32(1.0), 0, 0), (-1, np.float32(2.0), 0, 0)
    good = [(0, np.float32(0.0), 1, 2), L, R]
    trees = [good,
             [(0, np.float32(0.0), 0, 2), L, R],            # left child = the node itself
             [(0, np.float32(0.0), 1, -1), L, R],           # right child behind the node (the previous tree's last node)
             [(0, np.float32(0.0), 3, 2), L, R],            # left child = the tree's end (the next tree's root)
             [(0, np.float32(0.0), 1, 2 ** 31 - 1), L, R],  # right child far past everything: b + child is formed in 64 bits
             [(0, np.float32(0.0), -2 ** 31, 2), L, R],
             [(len(FEATS), np.float32(0.0), 1, 2), L, R],   # feature index == n_features
             [(0xFFFF, np.float32(0.0), 1, 2), L, R],
             [(1, np.float32(5.0), 1, 2), (1, np.float32(2.0), 0, 2), R, L],  # second level: a self loop on the left, fine on the right
             good]
    nodes = np.array([n for t in trees for n in t], dtype=NODE_DTYPE)
    sizes = [len(t) for t in trees]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    tab.check(FEATS, extra, (nodes, ptr, np.float32(0.25), LE), REPLACE, doc, score, count, [1, m], what="children and features")
    # tree ranges: empty, reversed, before the table, past its end -- each is +0, the good trees around them still count
    n = len(nodes)
    for bad_ptr in ([0, 3, 3, 6], [0, 3, 0, 3, 6], [0, 3, -5, 3, 6], [0, 3, n + 1, 3], [0, 3, n + 4, n + 9], [-3, 0, 3], [2 ** 31 - 1, -2 ** 31, 0, 3]):
        live, bits = tab.check(FEATS, extra, (nodes, np.array(bad_ptr, np.int32), np.float32(0.25), LE), SUM, doc, score, count, [m], what=bad_ptr)
    assert live.any()


# ---- 5. ties, NaNs, streams, reruns --------------------------------------------------------------------------------------------------
def test_nan_scores_rank_behind_minus_infinity(tab):
    m = 12
    doc = (np.arange(m)[::-1] + DOC_BASE + 100)[None, :].astype(np.int32).repeat(2, 0)
    score = np.array([[NAN, -np.inf, 1.0, 1.0, np.inf, -0.0, 0.0, NAN, -np.inf, 2.0, 1.0, -1.0]] * 2, np.float32)
    score[1] = np.float32(-np.inf)  # SUM with a finite model output: all -inf, the doc id decides
    zero = (np.array([(-1, 0.0, 0, 0)], dtype=NODE_DTYPE), np.array([0, 1], np.int32), np.float32(0.0), LE)
    live, bits = tab.check([(F_SCORE, 0)], None, zero, SUM, doc, score, None, [1, 5, m])
    od, ob, oc, op = ltr_ref.select(live, bits, doc, m)
    assert op[0].tolist() == [4, 9, 10, 3, 2, 6, 5, 11, 8, 1, 7, 0] and ob[0, -2:].tolist() == [0x7FC00000] * 2  # -0 + 0 is +0: the zeros tie; NaNs last, by doc id
    assert op[1].tolist() == list(range(m))[::-1]
    # a NaN the sum makes is stored canonical too: the model overflows to +inf where s <= 0, and -inf + inf is a NaN
    inf_leaf = (np.array([(0, 0.0, 1, 2), (-1, 3e38, 0, 0), (-1, -3e38, 0, 0)] * 2, dtype=NODE_DTYPE), np.array([0, 3, 6], np.int32), np.float32(3e38), LE)
    live, bits = tab.check([(F_SCORE, 0)], None, inf_leaf, SUM, doc, score, None, [m])
    assert (bits[1] == 0x7FC00000).all() and bits[0, 1] == 0x7FC00000


def test_side_stream_and_two_runs_into_the_same_buffers(tab):
    import torch
    m = 257
    rng = np.random.default_rng(18)
    nodes, ptr = forest(rng, 4, 3, len(FEATS), thresholds_of(tab.cols, FEATS, m))
    doc, score, count, extra = lists(19, NQ, m)
    model = (nodes, ptr, np.float32(0.5), LE)
    live, bits = tab.reference(FEATS, extra, model, REPLACE, doc, score, count)
    want = ltr_ref.select(live, bits, doc, 50)
    side = torch.cuda.Stream(device=DEVICE)
    for kw in (dict(stream=side), dict(twice=True), dict(stream=side, twice=True)):
        got = tab.run_topk(FEATS, extra, model, REPLACE, doc, score, count, 50, **kw)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), kw
    assert np.array_equal(tab.run_score(FEATS, extra, model, REPLACE, doc, score, count, stream=side), bits)


def test_no_columns_and_no_extra(tab):
    """n_cols == 0 with a NULL cols, and a NULL extra: legal when no feature names them"""
    bare = _Table([])
    rng = np.random.default_rng(20)
    feats = [(F_RANK, 0), (F_SCORE, 0)]
    nodes, ptr = forest(rng, 6, 3, 2, thresholds_of([], feats, 40))
    doc, score, count, _ = lists(21, NQ, 40)
    bare.check(feats, None, (nodes, ptr, np.float32(0.0), LE), REPLACE, doc, score, count, [1, 40])


def test_refusals_on_the_gpu_machine():
    from test_ltr_cpu import refusals
    refusals()


# ---- 6. a scikit-learn model --------------------------------------------------------------------------------------------------------
def test_sklearn_gbr_is_bit_equal_to_the_restatement(tab):
    pytest.importorskip("sklearn")
    from sklearn.ensemble import GradientBoostingRegressor
    from sparse_rx.ltr import ForestModel
    feats = [(F_SCORE, 0), (F_RANK, 0), (F_COLUMN, 0), (F_COLUMN, 3), (F_EXTRA, 0), (F_EXTRA, 1)]
    m = 40
    doc, score, count, extra = lists(22, NQ, m)
    rng = np.random.default_rng(23)
    X = np.stack([rng.integers(-8, 9, 800) / 4.0, rng.integers(0, m, 800), rng.integers(-50, 50, 800), rng.integers(0, 8, 800), rng.integers(-8, 9, 800) / 4.0,
                  rng.integers(-8, 9, 800) / 4.0], axis=1).astype(np.float32)
    y = X[:, 0] * 2 - 0.05 * X[:, 1] + (X[:, 2] > 10) + 0.3 * X[:, 3] * X[:, 4] + rng.standard_normal(800) * 0.1
    mdl = ForestModel.from_sklearn(GradientBoostingRegressor(n_estimators=40, max_depth=3, random_state=0).fit(X, y))
    assert mdl.n_trees == 40
    live, bits = tab.check(feats, extra, (mdl.nodes, mdl.tree_ptr, mdl.base, LE), REPLACE, doc, score, count, [1, 10, m])
    assert len(np.unique(bits[live])) > 50


# ---- 7. the Python doors -------------------------------------------------------------------------------------------------------------
def test_field_table_doors():
    import torch
    from sparse_rx import FieldTable
    from sparse_rx.ltr import ForestModel
    cols = table()
    columns = {"votes": np.ma.masked_array(cols[0][1], mask=~cols[0][2]), "big": cols[1][1], "price": np.ma.masked_array(cols[2][1], mask=~cols[2][2]),
               "small": cols[3][1], "tags": [["a"]] * N_DOCS}
    ft = FieldTable.from_columns(columns, device=DEVICE, doc_base=DOC_BASE)
    names = ["score", "rank", "votes", "big", "price", ("extra", 0), ("extra", 2), "small"]
    m = 65
    rng = np.random.default_rng(24)
    nodes, ptr = forest(rng, 6, 3, len(FEATS), thresholds_of(cols, FEATS, m))
    mdl = ForestModel.from_arrays(np.where(nodes["feature"] < 0, -1, nodes["feature"] & 0xFFFF), nodes["value"], nodes["left"], nodes["right"], ptr, base=0.75,
                                  cmp="lt", default_left=(nodes["feature"] >= 0) & ((nodes["feature"] & MISSING_LEFT) != 0))
    assert np.array_equal(mdl.nodes, nodes)
    doc, score, count, extra = lists(25, NQ, m)
    live, bits = ltr_ref.new_scores(cols, N_DOCS, DOC_BASE, FEATS, extra, nodes, ptr, np.float32(0.75), LT, SUM, doc, score, count)
    want = ltr_ref.select(live, bits, doc, 9)
    got = ft.rank_model(mdl, names, doc, score, count, 9, extra=extra, mode="sum", want_pos=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    dev = [torch.as_tensor(a, device=DEVICE) for a in (doc, score, count, extra)]
    out = ft.rank_model_device(mdl, names, *dev[:3], 9, extra=dev[3], mode="sum")
    assert len(out) == 3 and np.array_equal(out[0].cpu().numpy(), want[0])
    assert np.array_equal(ft.model_scores_device(mdl, names, *dev[:3], extra=dev[3], mode="sum").cpu().numpy().view(np.uint32), bits)
    bare = FieldTable.without_columns(N_DOCS, device=DEVICE, doc_base=DOC_BASE)
    leaf = ForestModel.from_arrays([0, -1, -1], [0.0, 1.0, 2.0], [1, 0, 0], [2, 0, 0], [0, 3])
    od, os_, oc = bare.rank_model(leaf, ["score"], doc, score, count, 3)
    w = ltr_ref.ltr_topk([], N_DOCS, DOC_BASE, [(F_SCORE, 0)], None, leaf.nodes, leaf.tree_ptr, leaf.base, LE, REPLACE, doc, score, count, 3)
    assert np.array_equal(od, w[0]) and np.array_equal(os_.view(np.uint32), w[1]) and np.array_equal(oc, w[2])
    for call, word in ((lambda: ft.rank_model_device(mdl, names, *dev[:3], 9), "extra must be a float32 tensor"),
                       (lambda: ft.rank_model_device(mdl, names, *dev[:3], 9, extra=dev[3][:, :, :2]), "the features need 3"),
                       (lambda: ft.rank_model_device(mdl, names, *dev[:3], 66, extra=dev[3]), "k must be in"),
                       (lambda: ft.rank_model_device(mdl, names, dev[0].long(), dev[1], dev[2], 9, extra=dev[3]), "int32 tensor"),
                       (lambda: ft.rank_model_device(mdl, names, dev[0].cpu(), dev[1], dev[2], 9, extra=dev[3]), "is on"),
                       (lambda: ft.rank_model_device(mdl, names, torch.zeros((1, 2049), dtype=torch.int32, device=DEVICE),
                                                     torch.zeros((1, 2049), device=DEVICE), None, 9), "1 to 2048"),
                       (lambda: ft.rank_model_device(mdl, names[:3], *dev[:3], 9), "the list has 3 features"),
                       (lambda: ft.rank_model_device(mdl, names[:7] + ["tags"], *dev[:3], 9, extra=dev[3]), "set column"),
                       (lambda: ft.rank_model_device(mdl, names, *dev[:3], 9, extra=dev[3], mode="multiply"), "mode must be"),
                       (lambda: bare.rank_model_device(mdl, names, *dev[:3], 9, extra=dev[3]), "needs doc fields"),
                       (lambda: ft.rank_model(mdl, names, doc, score, count, 9), "give extra")):
        with pytest.raises(ValueError, match=word):
            call()
    ft.close()


# ---- 8. end to end on text_small -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    ids = list(j["corpus"])
    rng = np.random.default_rng(3)
    return j, ids, {"price": (rng.random(len(ids)) * 50).astype(np.float32), "date": rng.integers(0, 10_000, len(ids)).astype(np.int64),
                    "tags": [["a"]] * len(ids)}


def _ref_rank_dict(results, mdl, feats, columns, names, row, top_k, extra=None, mode=REPLACE):
    """ltr_ref over result dicts: {qid: [(doc id, model score)]}; extra: {qid: f32[len, n_extra]}"""
    ref_cols = [(columns[nm].type, columns[nm].data, columns[nm].valid) for nm in names]
    n = len(row)
    out = {}
    for q, hits in results.items():
        ids = list(hits)
        if not ids:
            out[q] = []
            continue
        d = np.asarray([[row[i] for i in ids]], dtype=np.int32)
        s = np.asarray([[hits[i] for i in ids]], dtype=np.float32)
        od, ob, oc, op = ltr_ref.ltr_topk(ref_cols, n, 0, feats, None if extra is None else extra[q][None], mdl.nodes, mdl.tree_ptr, mdl.base,
                                          LE if mdl.cmp == "le" else LT, mode, d, s, None, min(top_k, len(ids)))
        out[q] = [(ids[p], float(b)) for p, b in zip(op[0, : oc[0]], ob[0, : oc[0]].view(np.float32))]
    return out


def _text_model(rng, n_features, thresholds, n_trees=12):
    from sparse_rx.ltr import ForestModel
    nodes, ptr = forest(rng, n_trees, 3, n_features, thresholds, leaf=lambda r: np.float32(r.standard_normal()))
    return ForestModel.from_arrays(np.where(nodes["feature"] < 0, -1, nodes["feature"] & 0xFFFF), nodes["value"], nodes["left"], nodes["right"], ptr, base=0.5,
                                   default_left=(nodes["feature"] >= 0) & ((nodes["feature"] & MISSING_LEFT) != 0))


def test_search_bm25_rank_model_end_to_end(text, tmp_path):
    import oracle
    import sparse_rx
    from sparse_rx.fields import host_columns
    from sparse_rx.ltr import ForestModel
    j, ids, fields = text
    queries = {q: j["queries"][q] for q in list(j["queries"])[:10]}
    row = {d: i for i, d in enumerate(ids)}
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    with pytest.raises(ValueError, match="set_rank_model"):
        svc.search_bm25(queries, top_k=5, rank_model=True)
    rng = np.random.default_rng(31)
    thr = [np.float32([0.5, 1, 2, 4, 8]), np.float32([1, 3, 10, 30]), fields["price"][:20], fields["date"][:20].astype(np.float32)]
    mdl = _text_model(rng, 4, thr)
    names, feats = ["score", "rank", "price", "date"], [(F_SCORE, 0), (F_RANK, 0), (F_COLUMN, 0), (F_COLUMN, 1)]
    svc.set_rank_model(mdl, names)
    with pytest.raises(ValueError, match=r"search_bm25\(rank_model=True\) needs the docs' fields"):
        svc.search_bm25(queries, top_k=5, rank_model=True)
    svc.set_doc_fields(fields)
    columns = host_columns(fields)
    # the oracle's ranking, 60 deep, as result dicts
    h = svc.host
    qids = [q for q in queries if queries[q].strip()]
    qp, qt, qw = sparse_rx.encode_queries([queries[q] for q in qids], h.vocabulary)
    ed, es, ec = oracle.search_batch(h.indptr, h.indices, h.data, h.doc_lengths, h.idf, qp, qt, qw, 60, 1.2, 0.75, h.avgdl)
    ranked = {q: {ids[int(ed[i, t])]: float(es[i, t]) for t in range(int(ec[i]))} for i, q in enumerate(qids)}
    pool = svc.search_bm25(queries, top_k=60)
    assert {q: list(v.items()) for q, v in pool.items() if q in ranked} == {q: list(v.items()) for q, v in ranked.items()}
    for top_k in (None, 5):
        got = svc.rerank_model(pool, top_k)
        want = _ref_rank_dict(ranked, mdl, feats, columns, ["price", "date"], row, 60 if top_k is None else top_k)
        assert all(list(got[q].items()) == want[q] for q in ranked), top_k
    got = svc.rerank_model(pool, 5, mode="sum")
    want = _ref_rank_dict(ranked, mdl, feats, columns, ["price", "date"], row, 5, mode=SUM)
    assert all(list(got[q].items()) == want[q] for q in ranked)
    same = lambda a, b: {q: list(v.items()) for q, v in a.items()} == {q: list(v.items()) for q, v in b.items()}
    # the keyword: pool-relative
    assert same(svc.search_bm25(queries, top_k=5, rank_model=True, rank_pool=60), svc.rerank_model(pool, 5))
    assert same(svc.search_bm25(queries, top_k=5, rank_model=True), svc.rerank_model(svc.search_bm25(queries, top_k=100), 5))
    kw = dict(excluded_docs=ids[:50], where={"must": [{"field": "date", "gte": 2000}]})
    assert same(svc.search_bm25(queries, top_k=4, rank_model=True, rank_pool=30, **kw), svc.rerank_model(svc.search_bm25(queries, top_k=30, **kw), 4))
    assert same(svc.search_bm25(queries, top_k=5, rank_model=False, rank_pool=7), svc.search_bm25(queries, top_k=5))
    # extras by doc id; a doc left out is missing
    m2 = _text_model(rng, 3, [np.float32([0.5, 1, 2]), np.float32([0.0, 0.5]), np.float32([0.0, 0.5])], n_trees=6)
    svc.set_rank_model(m2, ["score", ("extra", 0), ("extra", 1)])
    ex = {q: {d: [float(rng.integers(-4, 5)) / 4, float(rng.integers(-4, 5)) / 4] for d in list(v)[::2]} for q, v in pool.items()}
    planes = {q: np.array([ex[q].get(d, [np.nan, np.nan]) for d in v], np.float32).reshape(len(v), 2) for q, v in pool.items()}
    got = svc.rerank_model(pool, 7, extra=ex)
    want = _ref_rank_dict(pool, m2, [(F_SCORE, 0), (F_EXTRA, 0), (F_EXTRA, 1)], columns, [], row, 7, extra=planes)
    assert all(list(got[q].items()) == want[q] for q in pool)
    # a planted model: one stump on the date column moves a known doc to rank 1
    deep = svc.search_bm25({"q": queries[qids[0]]}, top_k=40)["q"]
    target = list(deep)[-1]
    date = fields["date"].copy()
    date[row[target]] = 20_000  # above every other date
    svc.set_doc_fields({**fields, "date": date})
    stump = ForestModel.from_arrays([0, -1, -1], [15_000.0, 0.0, 100.0], [1, 0, 0], [2, 0, 0], [0, 3])
    svc.set_rank_model(stump, ["date"])
    got = svc.search_bm25({"q": queries[qids[0]]}, top_k=3, rank_model=True, rank_pool=40)["q"]
    assert list(got)[0] == target and list(got.values()) == [100.0, 0.0, 0.0]
    assert list(got)[1:] == sorted((d for d in deep if d != target), key=row.get)[:2]  # equal scores: corpus order
    assert list(svc.search_bm25({"q": queries[qids[0]]}, top_k=3, rank_model=True, rank_pool=40, boost=None)["q"])[0] == target
    for bad, word in ((dict(boost={"functions": [{"decay": {"field": "date", "origin": 1, "scale": 1}}]}), "do not combine"), (dict(rank_pool=1025), "rank_pool")):
        with pytest.raises(ValueError, match=word):
            svc.search_bm25(queries, top_k=5, rank_model=True, **bad)
    svc.set_rank_model(stump, ["sparse_score"])
    with pytest.raises(ValueError, match="search_hybrid"):
        svc.search_bm25(queries, top_k=5, rank_model=True)
    svc.set_rank_model(stump, ["date"])
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.rerank_model({"q": {"no such doc": 1.0}})
    # the registry mirrors go through the same backend functions
    for r in (sparse_rx.OptimizedBM25Retriever(device=DEVICE, tile_log2=6), sparse_rx.OptimizedRetriever({"type": "bm25"}, device=DEVICE, tile_log2=6, cache_dir=str(tmp_path))):
        r.build_index_from_corpus(j["corpus"])
        r.set_doc_fields(fields)
        r.set_rank_model(mdl, names)
        one = {qids[1]: queries[qids[1]]}
        rpool = r.search(one, top_k=50)
        got = r.search(one, top_k=5, rank_model=True, rank_pool=50)
        want = _ref_rank_dict(rpool, mdl, feats, columns, ["price", "date"], row, 5)
        assert list(got[qids[1]].items()) == want[qids[1]] and same(got, r.rerank_model(rpool, 5))
        r.close()
    svc.close()


def test_search_hybrid_rank_model_uses_exact_scores_of_both_sides(text):
    import sparse_rx
    from sparse_rx.fields import host_columns
    j, ids, fields = text
    queries = {q: j["queries"][q] for q in list(j["queries"])[:10]}
    n_docs, dim = len(ids), 64
    rng = np.random.default_rng(47)
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    emb = rng.standard_normal((n_docs, dim)).astype(np.float32)
    svc.set_embeddings(emb)
    svc.set_doc_fields(fields)
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    columns, row = host_columns(fields), {d: i for i, d in enumerate(ids)}
    names = ["sparse_score", "dense_score", "score", "rank", "price"]
    thr = [np.float32([0.0, 1, 3, 6, 10]), np.float32([-8, -2, 0, 2, 8]), np.float32([0.1, 0.3, 0.6]), np.float32([2, 8, 20]), fields["price"][:20]]
    mdl = _text_model(rng, 5, thr)
    svc.set_rank_model(mdl, names)
    feats = [(F_EXTRA, 0), (F_EXTRA, 1), (F_SCORE, 0), (F_RANK, 0), (F_COLUMN, 0)]
    same = lambda a, b: {q: list(v.items()) for q, v in a.items()} == {q: list(v.items()) for q, v in b.items()}
    # the f32 dense index, then the half-precision one: "dense_score" is the score of the rounded rows there
    for storage, extra_kw in (("f32", dict()), ("f32", dict(rescore=True)), ("f32", dict(excluded_docs=ids[:40])), ("f16", dict()), ("f16", dict(rescore=True)),
                              ("bf16", dict())):
        if storage != getattr(svc, "embedding_storage", "f32"):
            svc.set_embeddings(emb, storage=storage)
        got = svc.search_hybrid(queries, vecs, top_k=5, rank_model=True, rank_pool=40, **extra_kw)
        pool = svc.search_hybrid(queries, vecs, top_k=40, **extra_kw)
        cands = {q: list(v) for q, v in pool.items()}
        sp, dn = svc.score_bm25(queries, cands), svc.score_by_vector(vecs, cands)
        planes = {q: np.array([[sp[q][d], dn[q][d]] for d in v], np.float32).reshape(len(v), 2) for q, v in pool.items()}
        want = _ref_rank_dict(pool, mdl, feats, columns, ["price"], row, 5, extra=planes)
        assert all(list(got[q].items()) == want[q] for q in queries), (storage, extra_kw)
        assert all(len(got[q]) == 5 for q in queries if queries[q].strip())
    svc.set_embeddings(emb)
    with pytest.raises(ValueError, match="cannot fill"):
        svc.set_rank_model(mdl, names[:4] + [("extra", 0)]) or svc.search_hybrid(queries, vecs, top_k=5, rank_model=True)
    # a model without the two names is the public chain; then collapse / MMR behind it
    svc.set_rank_model(_text_model(rng, 3, thr[2:]), ["score", "rank", "price"])
    got = svc.search_hybrid(queries, vecs, top_k=5, rank_model=True, rank_pool=40)
    assert same(got, svc.rerank_model(svc.search_hybrid(queries, vecs, top_k=40), 5))
    assert same(svc.search_hybrid(queries, vecs, top_k=5, rank_model=True), svc.rerank_model(svc.search_hybrid(queries, vecs, top_k=100), 5))
    got = svc.search_hybrid(queries, vecs, top_k=5, rank_model=True, rank_pool=40, mmr_lambda=0.5, mmr_pool=12)
    assert same(got, svc.diversify(svc.rerank_model(svc.search_hybrid(queries, vecs, top_k=40), 12), top_k=5, mmr_lambda=0.5))
    assert same(svc.search_hybrid(queries, vecs, top_k=5, rank_model=False, rank_pool=7), svc.search_hybrid(queries, vecs, top_k=5))
    for bad, word in ((dict(rank_pool=1025), "rank_pool must be in"), (dict(boost={"functions": [{"decay": {"field": "date", "origin": 1, "scale": 1}}]}), "do not combine")):
        with pytest.raises(ValueError, match=word):
            svc.search_hybrid(queries, vecs, top_k=5, rank_model=True, **bad)
    svc.close()
