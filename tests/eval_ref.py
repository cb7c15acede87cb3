"""Restatements of include/eval/sparse_rx_eval.h for the tests.

:func:`eval_lists` is the CONTRACT in NumPy: every operation rounded on its own to float32, the sums over the contributing
positions only and in ascending order (``np.add.accumulate`` adds strictly left to right), the means in float64 by chunks of 1 024
queries.  The GPU tests compare it with ``srx_eval_lists`` bit for bit.

:func:`eval_query_f64` is written from the metric definitions alone -- a dict of judgments, a Python list, Python floats -- and
shares no code with the first: the CPU test bounds the distance between the two by the rounding of fp32."""
import math

import numpy as np

NDCG, AP, RECALL, P, RR, SUCCESS, DCG, IDCG = range(8)
METRICS, MAX_M, MAX_K, MAX_GAIN = 8, 2048, 8, 32
WAVE_M, LDS_ROW, MEAN_CHUNK = 256, 1024, 1024
F32 = np.float32


def gain_table(kind: str, n_gain: int) -> np.ndarray:
    """"linear": g; "exp2": 2^g - 1 -- float64, rounded once to float32"""
    g = np.arange(n_gain, dtype=np.float64)
    return (g if kind == "linear" else np.exp2(g) - 1.0).astype(F32)


def discount_table(m: int) -> np.ndarray:
    """1 / log2(r + 2) of position r -- float64, rounded once to float32"""
    return (1.0 / np.log2(np.arange(m, dtype=np.float64) + 2.0)).astype(F32)


def ideal_of(j_ptr, j_grade) -> np.ndarray:
    """``j_ideal``: every row's grades in descending order"""
    out = np.empty(len(j_grade), dtype=np.int32)
    for r in range(len(j_ptr) - 1):
        b, e = int(j_ptr[r]), int(j_ptr[r + 1])
        out[b:e] = np.sort(np.asarray(j_grade[b:e], dtype=np.int32))[::-1]
    return out


def _ordered(terms: np.ndarray, where: np.ndarray, limits) -> list:
    """the fp32 sum of ``terms[where]`` over the positions below each limit, from +0, left to right"""
    idx = np.flatnonzero(where)
    run = np.add.accumulate(terms[idx].astype(F32), dtype=F32) if len(idx) else np.zeros(0, F32)
    out = []
    for lim in limits:
        cnt = int(np.searchsorted(idx, lim, side="left"))
        out.append(run[cnt - 1] if cnt else F32(0.0))
    return out


def eval_lists(j_ptr, j_doc, j_grade, j_ideal, gain, discount, rel_level, cand_doc, cand_count, q_row, ks, means=True, nnz=None):
    """-> dict(out f32[nq, n_k, 8], hits i32[nq, n_k], judged i32[nq, n_k], rel i32[nq], mean f64[n_k, 8], n int)"""
    j_ptr, j_doc, j_grade, j_ideal = (np.asarray(a) for a in (j_ptr, j_doc, j_grade, j_ideal))
    gain, discount = np.asarray(gain, dtype=F32), np.asarray(discount, dtype=F32)
    cand_doc = np.asarray(cand_doc, dtype=np.int32)
    nq, m = cand_doc.shape
    n_rows, n_gain, n_k = len(j_ptr) - 1, len(gain), len(ks)
    nnz = len(j_doc) if nnz is None else nnz
    out = np.zeros((nq, n_k, METRICS), dtype=F32)
    hits, judged = np.zeros((nq, n_k), dtype=np.int32), np.zeros((nq, n_k), dtype=np.int32)
    rel = np.zeros(nq, dtype=np.int32)
    evaluated = np.zeros(nq, dtype=bool)
    for q in range(nq):
        row = int(q_row[q]) if q_row is not None else q
        if not 0 <= row < n_rows:
            continue
        evaluated[q] = True
        live = m if cand_count is None else min(max(int(cand_count[q]), 0), m)
        b, e = int(j_ptr[row]), int(j_ptr[row + 1])
        if not 0 <= b <= e <= nnz:
            b = e = 0
        docs, grades = j_doc[b:e], np.clip(j_grade[b:e].astype(np.int64), 0, n_gain - 1)
        ideal = np.clip(j_ideal[b:e].astype(np.int64), 0, n_gain - 1)
        R = int((grades >= rel_level).sum())
        rel[q] = R
        # the join
        d = cand_doc[q, :live]
        at = np.searchsorted(docs, d, side="left")
        safe = np.minimum(at, max(len(docs) - 1, 0))
        J = (at < len(docs)) & (docs[safe] == d) if len(docs) else np.zeros(live, dtype=bool)
        g = np.where(J, grades[safe], 0) if len(docs) else np.zeros(live, dtype=np.int64)
        r = J & (g >= rel_level)
        gv = gain[g]
        n_s = [min(int(k), live) for k in ks]
        dcg = _ordered(gv * discount[:live], gv > 0, n_s)
        nid = min(len(ideal), m)
        iv = gain[ideal[:nid]]
        idcg = _ordered(iv * discount[:nid], iv > 0, [min(int(k), nid) for k in ks])
        through = np.cumsum(r)
        ap_terms = through.astype(F32) / (np.arange(live) + 1).astype(F32)
        ap = _ordered(ap_terms, r, n_s)
        relpos = np.flatnonzero(r)
        for ik, k in enumerate(ks):
            n = n_s[ik]
            h = int(r[:n].sum())
            hits[q, ik], judged[q, ik] = h, int(J[:n].sum())
            o = out[q, ik]
            o[NDCG] = F32(0.0) if idcg[ik] == 0 else dcg[ik] / idcg[ik]
            o[AP] = F32(0.0) if R == 0 else ap[ik] / F32(R)
            o[RECALL] = F32(0.0) if R == 0 else F32(h) / F32(R)
            o[P] = F32(h) / F32(int(k))
            o[RR] = F32(1.0) / F32(int(relpos[0]) + 1) if len(relpos) and relpos[0] < n else F32(0.0)
            o[SUCCESS] = F32(1.0) if h > 0 else F32(0.0)
            o[DCG], o[IDCG] = dcg[ik], idcg[ik]
    res = {"out": out, "hits": hits, "judged": judged, "rel": rel}
    if means:
        n = int(evaluated.sum())
        chunks = []
        for q0 in range(0, nq, MEAN_CHUNK):
            vals = out[q0:q0 + MEAN_CHUNK][evaluated[q0:q0 + MEAN_CHUNK]].astype(np.float64)
            chunks.append(np.add.accumulate(vals, axis=0)[-1] if len(vals) else np.zeros((n_k, METRICS)))
        total = np.add.accumulate(np.stack(chunks), axis=0)[-1] if chunks else np.zeros((n_k, METRICS))
        res["mean"] = total / float(n) if n else np.zeros((n_k, METRICS))
        res["n"] = n
    return res


def eval_query_f64(judgments: dict, ranking: list, k: int, gain: str = "linear", rel_level: int = 1, max_grade: int = 31, m=None):
    """One query from the definitions, in Python floats: ``judgments`` {doc: grade}, ``ranking`` the docs in rank order.  ``m``: the
    depth the lists are stored at (the ideal ranking is cut there too).  -> dict of the eight metrics plus hits / judged / rel."""
    def clamp(g):
        return min(max(g, 0), max_grade)

    def gain_of(g):
        return float(g) if gain == "linear" else 2.0 ** g - 1.0

    top = ranking[:k]
    n_rel = sum(1 for g in judgments.values() if clamp(g) >= rel_level)
    dcg = sum(gain_of(clamp(judgments[d])) / math.log2(i + 2) for i, d in enumerate(top) if d in judgments)
    best = sorted((clamp(g) for g in judgments.values()), reverse=True)[:k if m is None else min(k, m)]
    idcg = sum(gain_of(g) / math.log2(i + 2) for i, g in enumerate(best))
    flags = [d in judgments and clamp(judgments[d]) >= rel_level for d in top]
    n_hits = sum(flags)
    precisions = [sum(flags[:i + 1]) / (i + 1) for i, f in enumerate(flags) if f]
    return {"NDCG": dcg / idcg if idcg > 0 else 0.0, "AP": sum(precisions) / n_rel if n_rel else 0.0, "RECALL": n_hits / n_rel if n_rel else 0.0,
            "P": n_hits / k, "RR": 1.0 / (flags.index(True) + 1) if n_hits else 0.0, "SUCCESS": 1.0 if n_hits else 0.0, "DCG": dcg, "IDCG": idcg,
            "hits": n_hits, "judged": sum(1 for d in top if d in judgments), "rel": n_rel}
