"""NumPy restatement of include/sparse_rx_mmr.h, written from the header: which positions of a candidate list are live, the
two similarity modes on a given Gram matrix, the greedy selection in float32 with one rounding per operation and ties to the
lowest position, and the fp64 Gram matrix of given rows.  Never calls the engine."""
import numpy as np

DOT, COSINE = 0, 1  # srx_mmr_sim
MODES = {"dot": DOT, "cosine": COSINE}
MAX_M = 256
F = np.float32


def weights(lambda_):
    """(w_rel, w_div) as the Python layer derives them: float32(lambda_), float32(1 - lambda_) with the difference in double."""
    return F(float(lambda_)), F(1.0 - float(lambda_))


def live_mask(cand_doc, cand_rel, count, n_docs, doc_base):
    """bool[m]: c < min(max(count, 0), m) (count None = m), the id inside [doc_base, doc_base + n_docs), the relevance not NaN."""
    d = np.asarray(cand_doc, dtype=np.int64)
    m = d.shape[0]
    lim = m if count is None else min(max(int(count), 0), m)
    local = d - int(doc_base)
    return (np.arange(m) < lim) & (local >= 0) & (local < n_docs) & ~np.isnan(np.asarray(cand_rel, dtype=F))


def similarity_column(G, s, mode, norms=None):
    """S(c, s) for every c -- the candidate first, the picked doc s second: column s of G -- as float32[m]."""
    g = np.asarray(G, dtype=F)[:, s]
    if mode == DOT:
        return g
    d = norms * norms[s]  # float32 * float32: one rounding
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d > 0, g / np.where(d > 0, d, F(1.0)), F(0.0)).astype(F)  # float32 / float32: one rounding


def select(G, rel, live, k, w_rel, w_div, mode):
    """The selection of one query.  G: f32[m, m] (G[a, b] in its own orientation), rel f32[m], live bool[m].  Returns
    (positions picked, in order; v of each pick as float32).  Every array below is float32, so every elementwise operation
    is one float32 operation with one rounding."""
    G = np.asarray(G, dtype=F)
    rel = np.asarray(rel, dtype=F)
    w_rel, w_div = F(w_rel), F(w_div)
    is_open = np.asarray(live, dtype=bool).copy()
    norms = None
    if mode == COSINE:
        with np.errstate(invalid="ignore"):
            norms = np.sqrt(np.diagonal(G).astype(F))  # float32 in, float32 out: correctly rounded
    with np.errstate(invalid="ignore"):
        wr = w_rel * rel  # a dead position's value is never looked at
    assert wr.dtype == F
    pen = np.zeros_like(wr)
    picked, values = [], []
    while len(picked) < k and is_open.any():
        v = wr if not picked else wr - w_div * pen
        assert v.dtype == F
        idx = np.flatnonzero(is_open)
        best = int(idx[np.argmax(v[idx])])  # the first of equal maxima: the lowest position
        picked.append(best)
        values.append(v[best])
        is_open[best] = False
        S = similarity_column(G, best, mode, norms)
        pen = S if len(picked) == 1 else np.where(S > pen, S, pen)
    return picked, np.asarray(values, dtype=F)


def select_rows(G, cand_doc, cand_rel, cand_count, n_docs, doc_base, k, lambda_, mode):
    """The four outputs of a batch: G f32[nq, m, m] with the dead rows / columns ignored.  Returns (doc i32[nq, k], rel
    f32[nq, k], mmr f32[nq, k], count i32[nq]) padded with -1 / +0."""
    cand_doc, cand_rel = np.asarray(cand_doc), np.asarray(cand_rel, dtype=F)
    nq, m = cand_doc.shape
    w_rel, w_div = weights(lambda_)
    doc = np.full((nq, k), -1, np.int32)
    rel = np.zeros((nq, k), F)
    mmr = np.zeros((nq, k), F)
    count = np.zeros(nq, np.int32)
    for q in range(nq):
        live = live_mask(cand_doc[q], cand_rel[q], None if cand_count is None else cand_count[q], n_docs, doc_base)
        picked, values = select(G[q], cand_rel[q], live, k, w_rel, w_div, mode)
        n = len(picked)
        doc[q, :n], rel[q, :n], mmr[q, :n], count[q] = cand_doc[q, picked], cand_rel[q, picked], values, n
    return doc, rel, mmr, count


def mask_gram(G, live):
    """out_sim of one query: the entries with a dead row or column are +0.0f."""
    out = np.asarray(G, dtype=F).copy()
    out[~live, :] = 0.0
    out[:, ~live] = 0.0
    return out


def gram_exact(rows_a):
    """fp64 Gram matrix of the given rows: f64[m, m]."""
    x = np.asarray(rows_a, dtype=np.float64)
    return x @ x.T


def select_naive_f64(G, rel, live, k, w_rel, w_div, mode):
    """A second, deliberately naive restatement in fp64 (argmax over a score vector rebuilt at every step).  On inputs whose
    every intermediate is representable in float32 it must agree with :func:`select` exactly."""
    G = np.asarray(G, dtype=np.float64)
    rel = np.asarray(rel, dtype=np.float64)
    m = len(rel)
    if mode == COSINE:
        n = np.sqrt(np.diagonal(G))
        d = np.outer(n, n)
        S = np.where(d > 0, G / np.where(d > 0, d, 1.0), 0.0)
    else:
        S = G
    picked, values = [], []
    remaining = [c for c in range(m) if live[c]]
    while len(picked) < k and remaining:
        score = {c: float(w_rel) * rel[c] - (float(w_div) * max(S[c, s] for s in picked) if picked else 0.0) for c in remaining}
        top = max(score.values())
        best = min(c for c in remaining if score[c] == top)
        picked.append(best)
        values.append(score[best])
        remaining.remove(best)
    return picked, np.asarray(values, dtype=np.float64)
