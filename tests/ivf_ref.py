"""NumPy restatement of include/ivf/sparse_rx_ivf.h, written from the header: the arg-max, the probe order, the search over the
probed lists and the summation order of the centroid update.  Never calls the engine; scores come in from the caller (exact
integer dot products, or the engine's own scorer bits where the header pins a result to them)."""
import numpy as np

import half_ref


def rounded(x, dtype):
    """f32 values after the rounding to the index type."""
    return half_ref.to_f32(half_ref.round_codes(x, dtype), dtype)


def int_scores(q, d):
    """Exact dot products of small-integer operands as float32: f32[nq, n]."""
    return (np.asarray(q, np.float64) @ np.asarray(d, np.float64).T).astype(np.float32)


def assign(scores):
    """The column of the largest score, ties to the lowest column."""
    return np.argmax(scores, axis=1).astype(np.int32)


def probe(scores, nprobe):
    """(list i32[nq, nprobe], score f32[nq, nprobe]) by (score descending, list ascending), padded with -1 / +0."""
    nq, nlist = scores.shape
    pl, ps = np.full((nq, nprobe), -1, np.int32), np.zeros((nq, nprobe), np.float32)
    for q in range(nq):
        order = np.lexsort((np.arange(nlist), -scores[q].astype(np.float64)))[:nprobe]
        pl[q, : len(order)], ps[q, : len(order)] = order, scores[q, order]
    return pl, ps


def search(scores, doc_list, probe_list, k, score_offset=0.0, allowed=None, doc_base=0):
    """The rules of srx_ivf_search over scores f32[nq, n_docs]: docs of the probed lists (-1 and repeats skipped) that are
    allowed (bool[nq, n_docs] or None), value fl32(score + offset) > 0, order (value descending, doc ascending)."""
    nq, n = scores.shape
    doc, sc, cnt = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
    for q in range(nq):
        v = scores[q] + np.float32(score_offset)
        ok = np.isin(doc_list, probe_list[q][probe_list[q] >= 0]) & (v > 0)
        if allowed is not None:
            ok &= allowed[q]
        ids = np.flatnonzero(ok)
        ids = ids[np.lexsort((ids, -v[ids].astype(np.float64)))][:k]
        doc[q, : len(ids)], sc[q, : len(ids)], cnt[q] = ids + doc_base, v[ids], len(ids)
    return doc, sc, cnt


def update(rows, member_ptr, member, prev):
    """The header's order: per list, chunks of 256 members each summed sequentially from +0.0f, the partials added sequentially
    from +0.0f, an IEEE division by (float)count; an empty list keeps prev."""
    out = np.array(prev, np.float32)
    for c in range(len(member_ptr) - 1):
        m = member[member_ptr[c]: member_ptr[c + 1]]
        if len(m) == 0:
            continue
        total = np.zeros(rows.shape[1], np.float32)
        for lo in range(0, len(m), 256):
            part = np.zeros(rows.shape[1], np.float32)
            for r in m[lo: lo + 256]:
                part = part + rows[r]
            total = total + part
        out[c] = total / np.float32(len(m))
    return out
