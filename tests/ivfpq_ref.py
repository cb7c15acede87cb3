"""NumPy restatement of include/ivfpq/sparse_rx_ivfpq.h, composed from the parents' restatements: pq_ref (encode, lut, scores),
ivf_ref (rounding, probe, search) and half_ref through ivf_ref.  Rounded centroid -> residual -> codes -> fl(coarse + sum) -> the
search and score-docs rules.  Never calls the engine; the coarse terms come in from the caller (exact integer dot products)."""
import numpy as np

import ivf_ref
import pq_ref

probe, search, score_docs = ivf_ref.probe, ivf_ref.search, pq_ref.score_docs


def residuals(x, lists, cent, dtype):
    """r = fl(x - c): c the f32 value of the rounded centroid of the row's list."""
    return np.asarray(x, np.float32) - ivf_ref.rounded(np.asarray(cent, np.float32), dtype)[lists]


def codes(x, lists, cent, dtype, cb):
    return pq_ref.encode(residuals(x, lists, cent, dtype), cb)


def scores(q, coarse, lists, code, cb):
    """f32[nq, n]: fl(coarse[q][list(d)] + s), s the sequential sum of the table entries (one table per query)."""
    return np.asarray(coarse, np.float32)[:, lists] + pq_ref.scores(pq_ref.lut(q, cb), code)


def reconstruct(code, lists, cent, dtype, cb, dim):
    return ivf_ref.rounded(np.asarray(cent, np.float32), dtype)[lists] + pq_ref.reconstruct(code, cb, dim)
