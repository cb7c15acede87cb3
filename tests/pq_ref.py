"""NumPy restatement of the arithmetic of include/pq/sparse_rx_pq.h, written from its text: every step is ONE float32 operation,
the loops run over j / m in the header's order and are vectorised over everything else."""
import numpy as np


def subspaces(dim, dsub):
    return -(-dim // dsub)


def _padded(x, M, dsub):
    out = np.zeros((x.shape[0], M * dsub), np.float32)
    out[:, : x.shape[1]] = x
    return out.reshape(x.shape[0], M, dsub)


def encode(x, cb):
    """u8[n, M]: best = +inf, code = 0; for c ascending, d(c) < best takes over (lowest code on ties, a NaN never wins)."""
    M, K, dsub = cb.shape
    xs = _padded(np.asarray(x, np.float32), M, dsub)
    best, code = np.full(xs.shape[:2], np.inf, np.float32), np.zeros(xs.shape[:2], np.uint8)
    with np.errstate(all="ignore"):
        for c in range(K):
            d = np.zeros(xs.shape[:2], np.float32)
            for j in range(dsub):
                t = xs[:, :, j] - cb[None, :, c, j]
                d = d + t * t
            take = d < best
            best, code = np.where(take, d, best), np.where(take, np.uint8(c), code)
    return code


def lut(q, cb):
    """f32[nq, M, 256]: the sequential sum from +0.0f over j ascending of fl(q[m dsub + j] * C[m][c][j])."""
    M, K, dsub = cb.shape
    qs = _padded(np.asarray(q, np.float32), M, dsub)
    out = np.zeros((qs.shape[0], M, K), np.float32)
    for j in range(dsub):
        out = out + qs[:, :, None, j] * cb[None, :, :, j]
    return out


def scores(table, codes):
    """f32[nq, n]: the sequential sum from +0.0f over m ascending of LUT[q][m][code[d][m]]."""
    out = np.zeros((table.shape[0], codes.shape[0]), np.float32)
    for m in range(codes.shape[1]):
        out = out + table[:, m, :][:, codes[:, m]]
    return out


def search(S, k, score_offset=0.0, allowed=None, doc_base=0):
    """The rules of srx_pq_search over scores f32[nq, n]: value fl32(score + offset) > 0, allowed (bool[nq, n] or None), order
    (value descending, doc ascending), padding -1 / +0.0f."""
    nq, n = S.shape
    doc, sc, cnt = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
    for q in range(nq):
        v = S[q] + np.float32(score_offset)
        ok = v > 0
        if allowed is not None:
            ok &= allowed[q]
        ids = np.flatnonzero(ok)
        ids = ids[np.lexsort((ids, -v[ids].astype(np.float64)))][:k]
        doc[q, : len(ids)], sc[q, : len(ids)], cnt[q] = ids + doc_base, v[ids], len(ids)
    return doc, sc, cnt


def score_docs(S, cand_doc, cand_count=None, doc_base=0):
    """f32[nq, m]: S at the given GLOBAL ids; +0.0f for padding, entries at or beyond the count and ids outside the corpus."""
    out = np.zeros(cand_doc.shape, np.float32)
    for q in range(cand_doc.shape[0]):
        lim = cand_doc.shape[1] if cand_count is None else min(cand_doc.shape[1], max(int(cand_count[q]), 0))
        local = cand_doc[q, :lim].astype(np.int64) - doc_base
        ok = (local >= 0) & (local < S.shape[1])
        out[q, :lim][ok] = S[q, local[ok]]
    return out


def reconstruct(codes, cb, dim):
    return cb[np.arange(cb.shape[0])[None, :], codes].reshape(codes.shape[0], -1)[:, :dim]
