"""NumPy restatement of include/sparse_rx_maxsim.h, written from the header: which positions and query tokens are live, the
max / ordered fp32 sum over a GIVEN similarity matrix, the ranking rule, the fp64 form of the score and the derived error
bound.  Never calls the engine; the roundings and the per-similarity bound are tests/half_ref.py's."""
import numpy as np

import half_ref

MAX_QT = 128   # SRX_MAXSIM_MAX_QT
MAX_M = 1024   # SRX_MAX_K: candidates per list of the rerank form


def shape_ok(tq, dim_pad):
    return 1 <= tq <= MAX_QT and (tq + 31) // 32 * 32 * dim_pad <= 32768


def live_positions(cand_doc_row, cand_count, doc_base, n_docs):
    """bool[m]: position c is live iff c < min(max(count, 0), m) (None: m) and the id is in [doc_base, doc_base + n_docs)."""
    d = np.asarray(cand_doc_row, dtype=np.int64)
    m = len(d)
    lim = m if cand_count is None else min(max(int(cand_count), 0), m)
    return (np.arange(m) < lim) & (d - doc_base >= 0) & (d - doc_base < n_docs)


def live_tokens(q_tok_count, tq):
    """How many query tokens of a query are live: min(max(count, 0), tq); None means tq."""
    return tq if q_tok_count is None else min(max(int(q_tok_count), 0), tq)


def score_from_sim(sim, n_live):
    """The score of one (query, doc) pair from sim f32[tq, t_d] (query token i, doc token j): M(i) = max_j sim(i, j), then
    (((+0 + M(0)) + M(1)) + ...) over i < n_live, one float32 add at a time.  A doc without tokens or a query without live
    tokens scores +0."""
    sim = np.asarray(sim, dtype=np.float32)
    if sim.ndim != 2 or sim.shape[1] == 0 or n_live <= 0:
        return np.float32(0.0)
    M = sim.max(axis=1)
    s = np.float32(0.0)
    for i in range(n_live):
        s = np.float32(s + M[i])
    return s


def rank(cand_doc_row, scores_row, live, k):
    """The rerank rule: the live positions by (score descending, doc ascending), cut to k.  Returns (doc i32[k] padded with -1,
    score f32[k] padded with +0, count)."""
    d = np.asarray(cand_doc_row, dtype=np.int64)
    s = np.asarray(scores_row, dtype=np.float32)
    pos = sorted(np.flatnonzero(live).tolist(), key=lambda c: (-float(s[c]), int(d[c])))[:k]
    out_d, out_s = np.full(k, -1, np.int32), np.zeros(k, np.float32)
    out_d[: len(pos)] = d[pos]
    out_s[: len(pos)] = s[pos]
    return out_d, out_s, len(pos)


def score_f64(q_codes, d_codes, dtype, n_live):
    """sum over the live query tokens of the largest fp64 dot product of the ROUNDED operands.  q_codes u16[tq, dim_pad],
    d_codes u16[t_d, dim_pad]."""
    if len(d_codes) == 0 or n_live <= 0:
        return 0.0
    return float(half_ref.exact_scores(q_codes[:n_live], d_codes, dtype).max(axis=1).sum())


def tol(q_codes, d_codes, dtype, n_live):
    """sum_i max_j half_ref.tol(i, j) + tq * 2^-24 * sum_i |M(i)| over the live query tokens i (tq = len(q_codes)).
    Derivation: the max of perturbed values moves by at most the largest perturbation, so M(i) is within max_j tol(i, j) of
    its fp64 value; each of the (at most tq) ordered fp32 adds rounds a partial sum bounded by sum_i |M(i)| (relative 2^-24)."""
    if len(d_codes) == 0 or n_live <= 0:
        return 0.0
    t = half_ref.tol(q_codes[:n_live], d_codes, dtype).max(axis=1)
    M = np.abs(half_ref.exact_scores(q_codes[:n_live], d_codes, dtype).max(axis=1))
    return float(t.sum() + len(q_codes) * 2.0 ** -24 * M.sum())
