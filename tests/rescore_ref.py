"""NumPy restatement of the hybrid rescoring contracts (include/sparse_rx_rescore.h), written from
the contract's text: the three dense "score these docs" formulas with fp32 arrays (every multiply and add rounded to fp32
on its own -- NumPy's elementwise ufuncs do not fuse them) and the lane butterfly spelled out, and ``fuse_scored`` as a
dict per query with ``np.float32`` scalars, in the style of tests/hybrid_ref.py.  The GPU tests compare bit for bit."""
import numpy as np

from hybrid_ref import _used

F32 = np.float32


def live_candidates(cand_doc, cand_count, n_docs: int, doc_base: int = 0):
    """(live bool[nq, m], local row int64[nq, m]): entry c of row q is live iff c < max(cand_count[q], 0) (no cand_count:
    always) and cand_doc - doc_base, in 64 bits, lies in [0, n_docs).  Everything else scores +0."""
    cand_doc = np.asarray(cand_doc)
    nq, m = cand_doc.shape
    local = cand_doc.astype(np.int64) - int(doc_base)
    lim = np.full(nq, m, np.int64) if cand_count is None else np.maximum(np.asarray(cand_count).astype(np.int64), 0)
    live = (np.arange(m)[None, :] < lim[:, None]) & (local >= 0) & (local < n_docs)
    return live, local


def lane_dot(e, q):
    """e f32[n, dim] (rows as the kernel sees them after de-quantization), q f32[dim]; dim a multiple of 64.  Lane l holds
    p_l = (((+0 + e[l] * q[l]) + e[l + 64] * q[l + 64]) + ...), then for o = 32 .. 1 every lane takes a_l + a_(l xor o);
    the score is lane 0's value."""
    e, q = np.asarray(e, F32), np.asarray(q, F32)
    assert e.shape[1] % 64 == 0 and q.shape == (e.shape[1],)
    lanes = np.arange(64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        p = np.zeros((e.shape[0], 64), F32)
        for i in range(e.shape[1] // 64):
            p = p + e[:, 64 * i: 64 * i + 64] * q[64 * i: 64 * i + 64]
        for o in (32, 16, 8, 4, 2, 1):
            p = p + p[:, lanes ^ o]
    assert p.dtype == F32
    return p[:, 0]


def _gather(score_rows, nq, cand_doc, cand_count, n_docs, doc_base):
    """out f32[nq, m]: score_rows(q, rows int64[n]) -> f32[n] for the live candidates of query q, +0 elsewhere"""
    live, local = live_candidates(cand_doc, cand_count, n_docs, doc_base)
    assert live.shape[0] == nq
    out = np.zeros(live.shape, F32)
    for q in range(nq):
        if live[q].any():
            out[q, live[q]] = score_rows(q, local[q, live[q]])
    return out


def f32_scores(emb, queries, cand_doc, cand_count=None, doc_base=0):
    """srx_dense_score_docs_f32: emb f32[n_docs, dim], queries f32[nq, dim], dim a multiple of 64"""
    emb, queries = np.asarray(emb, F32), np.asarray(queries, F32)
    return _gather(lambda q, rows: lane_dot(emb[rows], queries[q]), len(queries), cand_doc, cand_count, len(emb), doc_base)


def u8_scores(corpus_u8, corpus_scales, queries_f32, cand_doc, cand_count=None, doc_base=0):
    """srx_dense_score_docs_u8: e = (float)u8 * corpus_scales[2 d] + corpus_scales[2 d + 1] (two roundings), then as f32"""
    c, s, queries = np.asarray(corpus_u8), np.asarray(corpus_scales, F32).reshape(-1), np.asarray(queries_f32, F32)
    assert c.dtype == np.uint8 and s.size == 2 * len(c)

    def rows_of(q, rows):
        e = c[rows].astype(F32) * s[2 * rows][:, None] + s[2 * rows + 1][:, None]
        assert e.dtype == F32
        return lane_dot(e, queries[q])

    return _gather(rows_of, len(queries), cand_doc, cand_count, len(c), doc_base)


def i8_scores(corpus_i8, corpus_scale, queries_i8, query_scale, cand_doc, cand_count=None, doc_base=0):
    """srx_dense_score_docs_i8: the exact integer dot, then (float)(((double)acc * (double)query_scale) * (double)corpus_scale)"""
    c, queries = np.asarray(corpus_i8), np.asarray(queries_i8)
    assert c.dtype == np.int8 and queries.dtype == np.int8
    cs, qs = np.asarray(corpus_scale, F32).astype(np.float64), np.asarray(query_scale, F32).astype(np.float64)

    def rows_of(q, rows):
        acc = c[rows].astype(np.int64) @ queries[q].astype(np.int64)
        return ((acc.astype(np.float64) * qs[q]) * cs[rows]).astype(F32)

    return _gather(rows_of, len(queries), cand_doc, cand_count, len(c), doc_base)


def packed_offsets(d: int, dim: int):
    """Byte offsets of row d's 16-byte pieces in the fragment order of srx_dense_pack_i8, piece p = bytes [16 p, 16 p + 16)
    of the row: with T = d / 32, s = p / 2, h = p % 2 the piece sits at ((T * dim / 32 + s) * 64 + (d & 31) + 32 h) * 16."""
    return [(((d // 32) * (dim // 32) + p // 2) * 64 + (d & 31) + 32 * (p % 2)) * 16 for p in range(dim // 16)]


def pack_i8(rows):
    """The fragment-order copy of i8[n, dim] rows (rows past n in the last tile of 32 are zeros)"""
    rows = np.asarray(rows, np.int8)
    n, dim = rows.shape
    out = np.zeros((n + 31) // 32 * 32 * dim, np.int8)
    for d in range(n):
        for p, off in enumerate(packed_offsets(d, dim)):
            out[off: off + 16] = rows[d, 16 * p: 16 * p + 16]
    return out


# ---- fusion of two completed lists ---------------------------------------------------------------------------------------
def fuse_scored_row(a_doc, a_score, a_other, a_count, b_doc, b_score, b_other, b_count, k, wa, wb):
    """One query: ranked [(doc, fused score f32)], at most k entries, fused score > 0 only."""
    ua, ub = _used(a_doc, a_score, a_count, len(a_doc)), _used(b_doc, b_score, b_count, len(b_doc))
    ma = F32(a_score[0]) if 0 in ua else None  # a side whose head is not used has no normaliser: it contributes nothing
    mb = F32(b_score[0]) if 0 in ub else None
    wa, wb = F32(wa), F32(wb)

    def contribution(s, w, m):
        if m is None or not (s > 0):  # NaN, zeros and negative values do not contribute
            return None
        return F32(w * F32(F32(s) / m))

    def fused_of(from_a, from_b):
        if from_a is None or from_b is None:
            return from_a if from_b is None else from_b
        return F32(from_a + from_b)

    fused = {}
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for r in ua:
            fused[int(a_doc[r])] = fused_of(contribution(a_score[r], wa, ma), contribution(a_other[r], wb, mb))
        in_a = set(fused)
        for r in ub:
            if int(b_doc[r]) in in_a:  # a doc in both lists is taken once, from list A
                continue
            fused[int(b_doc[r])] = fused_of(contribution(b_other[r], wa, ma), contribution(b_score[r], wb, mb))
    rows = [(d, s) for d, s in fused.items() if s is not None and s > 0]
    rows.sort(key=lambda t: (-int(F32(t[1]).view(np.uint32)), t[0]))  # positive floats: bit order = value order
    return rows[:k]


def fuse_scored(a, a_other, b, b_other, k, weights=(0.3, 0.7)):
    """Batch form with the engine's output layout: (doc i32[nq, k], score f32[nq, k], count i32[nq]), padded -1 / 0."""
    (a_doc, a_score, a_count), (b_doc, b_score, b_count) = a, b
    nq = len(a_count)
    doc = np.full((nq, k), -1, np.int32)
    score = np.zeros((nq, k), F32)
    count = np.zeros(nq, np.int32)
    for q in range(nq):
        rows = fuse_scored_row(a_doc[q], a_score[q], a_other[q], a_count[q], b_doc[q], b_score[q], b_other[q], b_count[q], k,
                               weights[0], weights[1])
        count[q] = len(rows)
        for r, (d, s) in enumerate(rows):
            doc[q, r], score[q, r] = d, s
    return doc, score, count


def others_from_lists(a, b):
    """The *_other arrays that make the scored fusion the plain weighted one: the opposite list's own score where the doc
    is a used entry of it, 0 elsewhere."""
    def one(x, y):
        (x_doc, _, x_count), (y_doc, y_score, y_count) = x, y
        out = np.zeros(x_doc.shape, F32)
        for q in range(len(x_count)):
            theirs = {int(y_doc[q][r]): y_score[q][r] for r in _used(y_doc[q], y_score[q], y_count[q], y_doc.shape[1])}
            for r in range(x_doc.shape[1]):
                out[q, r] = theirs.get(int(x_doc[q, r]), 0.0)
        return out
    return one(a, b), one(b, a)
