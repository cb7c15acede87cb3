"""include/ltr/sparse_rx_ltr.h restated in NumPy scalars and plain Python: the yardstick of tests/test_ltr_cpu.py and
tests/test_ltr_gpu.py.  Written from the header's contract, one candidate and one tree at a time; nothing here is fast."""
import numpy as np

F_SCORE, F_RANK, F_COLUMN, F_EXTRA = 0, 1, 2, 3
LE, LT = 0, 1
REPLACE, SUM = 0, 1
MISSING_LEFT = 1 << 30
MAX_M, MAX_COLS, MAX_FEATURES, MAX_EXTRA, MAX_TREES, MAX_NODES = 2048, 8, 32, 32, 4096, 1 << 22
I32, I64, F32, SET64 = 0, 1, 2, 3
NODE_DTYPE = np.dtype([("feature", "<i4"), ("value", "<f4"), ("left", "<i4"), ("right", "<i4")])
NODE_BYTES, FEATURE_BYTES = 16, 8
NAN_BITS = 0x7FC00000
F32_NAN = np.float32(np.nan)


def f32_bits(x) -> int:
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def order_map(bits: int) -> int:
    """The order-mapped bits of a score: larger = ranks earlier; every NaN maps to 0, behind -inf"""
    if (bits & 0x7FFFFFFF) > 0x7F800000:
        return 0
    return (~bits & 0xFFFFFFFF) if bits >> 31 else bits | 0x80000000


def feature_value(kind, index, cols, local, s, c, extra_row):
    """Feature (kind, index) of the live candidate at position c with the local doc `local` and the raw score s; cols = [(type,
    data, valid bool array | None)], extra_row = the plane's f32[n_extra] of this position (or None)"""
    if kind == F_SCORE:
        return np.float32(s)
    if kind == F_RANK:
        return np.float32(c)
    if kind == F_EXTRA:
        return np.float32(extra_row[index])
    typ, data, valid = cols[index]
    if valid is not None and not valid[local]:
        return F32_NAN
    if typ == F32:
        return np.float32(data[local])
    return np.asarray(data[local]).astype(np.float32)[()]  # int32 / int64 -> fp32, round to nearest even


def tree_output(nodes, b, e, n_nodes, n_features, cmp, x, want_leaf=False):
    """The contribution of the tree over nodes [b, e) for the feature vector x (steps 1 .. 6 of the header); with want_leaf the
    pair (contribution, index of the leaf reached relative to b, or -1)"""
    zero = np.float32(0.0)
    out = lambda v, leaf: (v, leaf) if want_leaf else v
    if not (0 <= b < e <= n_nodes):
        return out(zero, -1)
    i = b
    while True:
        nd = nodes[i]
        feat = int(nd["feature"])
        if feat < 0:
            return out(np.float32(nd["value"]), i - b)
        fi = feat & 0xFFFF
        if fi >= n_features:
            return out(zero, -1)
        xv, v = np.float32(x[fi]), np.float32(nd["value"])
        if np.isnan(xv):
            left = bool(feat & MISSING_LEFT)
        else:
            left = bool(xv <= v) if cmp == LE else bool(xv < v)
        j = b + int(nd["left"] if left else nd["right"])
        if not (i < j < e):
            return out(zero, -1)
        i = j


def model_score(nodes, tree_ptr, base, cmp, mode, n_features, x, s):
    """The new score of one candidate: acc = base, then one fp32 add per tree in order"""
    n_nodes = len(nodes)
    acc = np.float32(base)
    with np.errstate(all="ignore"):
        for t in range(len(tree_ptr) - 1):
            acc = np.float32(acc + tree_output(nodes, int(tree_ptr[t]), int(tree_ptr[t + 1]), n_nodes, n_features, cmp, x))
        return acc if mode == REPLACE else np.float32(np.float32(s) + acc)


def leaves(nodes, tree_ptr, cmp, n_features, x):
    """The leaf every tree reaches for x (index relative to the tree's first node; -1: none)"""
    return [tree_output(nodes, int(tree_ptr[t]), int(tree_ptr[t + 1]), len(nodes), n_features, cmp, x, want_leaf=True)[1]
            for t in range(len(tree_ptr) - 1)]


def new_scores(cols, n_docs, doc_base, features, extra, nodes, tree_ptr, base, cmp, mode, cand_doc, cand_score, cand_count):
    """(live bool[nq, m], bits uint32[nq, m]): which positions are live and the stored bits of their new scores (0 at the dead ones)"""
    nq, m = cand_doc.shape
    live = np.zeros((nq, m), dtype=bool)
    bits = np.zeros((nq, m), dtype=np.uint32)
    for q in range(nq):
        n = m if cand_count is None else min(max(int(cand_count[q]), 0), m)
        for c in range(n):
            local = int(cand_doc[q, c]) - int(doc_base)
            if not (0 <= local < n_docs):
                continue
            s = cand_score[q, c]
            x = [feature_value(kind, index, cols, local, s, c, None if extra is None else extra[q, c]) for kind, index in features]
            ns = model_score(nodes, tree_ptr, base, cmp, mode, len(features), x, s)
            live[q, c] = True
            bits[q, c] = NAN_BITS if np.isnan(ns) else f32_bits(ns)
    return live, bits


def ltr_score(*args):
    """srx_ltr_score: uint32 bits [nq, m]"""
    return new_scores(*args)[1]


def ltr_topk(cols, n_docs, doc_base, features, extra, nodes, tree_ptr, base, cmp, mode, cand_doc, cand_score, cand_count, k):
    """srx_ltr_topk: (out_doc i32[nq, k], out_score bits u32[nq, k], out_count i32[nq], out_pos i32[nq, k])"""
    return select(*new_scores(cols, n_docs, doc_base, features, extra, nodes, tree_ptr, base, cmp, mode, cand_doc, cand_score, cand_count), cand_doc, k)


def select(live, bits, cand_doc, k):
    """The selection of srx_ltr_topk over the (live, bits) of :func:`new_scores`"""
    nq, m = cand_doc.shape
    out_doc, out_pos = np.full((nq, k), -1, np.int32), np.full((nq, k), -1, np.int32)
    out_bits, out_count = np.zeros((nq, k), np.uint32), np.zeros(nq, np.int32)
    for q in range(nq):
        order = sorted((c for c in range(m) if live[q, c]), key=lambda c: (-order_map(int(bits[q, c])), int(cand_doc[q, c])))[:k]
        out_count[q] = len(order)
        for t, c in enumerate(order):
            out_doc[q, t], out_bits[q, t], out_pos[q, t] = cand_doc[q, c], bits[q, c], c
    return out_doc, out_bits, out_count, out_pos
