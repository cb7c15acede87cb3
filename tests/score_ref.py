"""NumPy restatement of the walk ``srx_score_docs`` (csrc/score_docs.hip) makes over the blocked layout, shared by the CPU
and GPU suites of the candidate scoring.

For every (query, candidate) pair and every query term in the query's order: the term's postings inside the doc's tile
are ``[term_ptr[t] + skip[t][j], term_ptr[t] + skip[t][j + 1])`` (padded positions; ``j = local doc >> tile_log2``), a
lower-bound search with UNSIGNED compares finds the doc there -- canonical sentinels are negative, compact ones are local
ids >= 49152, so both sort behind every real id and the range is ascending as it stands -- and a hit adds
``(v * idf[t]) * qw`` to the running fp32 sum.  In the compact copy the key is ``doc - first doc of its unit``.
"""
import numpy as np


def _flat_views(post, val_dtype, compact):
    """(keys u32[4 * blocks], values f32[4 * blocks]) by padded position, from the canonical blocks or the compact copy."""
    f32v = val_dtype == np.float32
    words = (6 if f32v else 4) if compact else (8 if f32v else 6)
    b = np.ascontiguousarray(np.asarray(post, np.int32).reshape(-1, words))
    if compact:
        keys = np.ascontiguousarray(b[:, :2]).view(np.uint16).astype(np.uint32).reshape(-1)
        vw = np.ascontiguousarray(b[:, 2:])
    else:
        keys = np.ascontiguousarray(b[:, :4]).view(np.uint32).reshape(-1)
        vw = np.ascontiguousarray(b[:, 4:])
    vals = vw.view(np.float32).reshape(-1) if f32v else vw.view(np.float16).astype(np.float32).reshape(-1)
    return keys, vals


def np_score_docs(term_ptr, post, tile_skip, idf, n_docs, tile_log2, unit_tiles, q_ptr, q_term, q_weight, cand_doc,
                  cand_count=None, doc_base=0, val_dtype=np.float32, compact=False):
    """``srx_score_docs`` restated: f32[nq, m].  ``post`` is the copy to walk (``compact``: parity.np_compact_blocks' output)."""
    f = np.float32
    G = 1 << tile_log2
    n_tiles = (n_docs + G - 1) >> tile_log2
    keys, vals = _flat_views(post, val_dtype, compact)
    term_ptr = np.asarray(term_ptr, np.int64)
    skip = np.asarray(tile_skip, np.int32).reshape(-1, n_tiles + 1)
    idf = np.asarray(idf, f)
    cand = np.asarray(cand_doc, np.int32)
    nq, m = cand.shape
    out = np.zeros((nq, m), f)
    for q in range(nq):
        local = cand[q].astype(np.int64) - int(doc_base)
        live = (local >= 0) & (local < n_docs)
        if cand_count is not None:
            live &= np.arange(m) < max(int(cand_count[q]), 0)
        idx = np.flatnonzero(live)
        if len(idx) == 0:
            continue
        loc = local[idx]
        j = loc >> tile_log2
        key = (loc - (j // unit_tiles) * (unit_tiles * G) if compact else loc).astype(np.uint32)
        s = np.zeros(len(idx), f)
        for i in range(int(q_ptr[q]), int(q_ptr[q + 1])):
            t = int(q_term[i])
            lo = term_ptr[t] + skip[t, j].astype(np.int64)
            end = term_ptr[t] + skip[t, j + 1].astype(np.int64)
            hi = end.copy()
            while np.any(lo < hi):
                open_ = lo < hi
                mid = lo + ((hi - lo) >> 1)
                right = keys[mid] < key
                lo = np.where(open_ & right, mid + 1, lo)
                hi = np.where(open_ & ~right, mid, hi)
            hit = (lo < end) & (keys[lo] == key)  # position `end` is inside the array: sentinel blocks follow the last run
            contrib = (vals[lo] * idf[t]) * f(q_weight[i])
            s = np.where(hit, s + contrib, s).astype(f)
        out[q, idx] = s
    return out


def oracle_full_scores(oracle, indptr, indices, data, doc_lengths, idf, q_ptr, q_term, q_weight, k1=1.2, b=0.75, avgdl=1.0,
                       tfidf=False):
    """f32[nq, n_docs]: ``oracle.scores_given_order`` of every query of a CSR batch (contributions in the batch's term order)."""
    nq = len(q_ptr) - 1
    n = len(indptr) - 1
    out = np.zeros((nq, n), np.float32)
    for q in range(nq):
        lo, hi = int(q_ptr[q]), int(q_ptr[q + 1])
        if hi > lo:
            out[q] = oracle.scores_given_order(indptr, indices, data, doc_lengths, idf, q_term[lo:hi], q_weight[lo:hi], k1, b, avgdl,
                                               tfidf=tfidf)
    return out


def gather_expected(full, cand_doc, cand_count=None, doc_base=0):
    """The contract's output for a candidate block, from full score vectors f32[nq, n_docs]: the doc's score, ``+0`` for
    padding and for ids outside [doc_base, doc_base + n_docs)."""
    cand = np.asarray(cand_doc, np.int64)
    nq, m = cand.shape
    n = full.shape[1]
    local = cand - int(doc_base)
    live = (local >= 0) & (local < n)
    if cand_count is not None:
        live &= np.arange(m)[None, :] < np.maximum(np.asarray(cand_count, np.int64), 0)[:, None]
    out = np.zeros((nq, m), np.float32)
    qq, cc = np.nonzero(live)
    out[qq, cc] = full[qq, local[qq, cc]]
    return out


def assert_bits_equal(got, exp, label=""):
    got = np.ascontiguousarray(got, dtype=np.float32)
    exp = np.ascontiguousarray(exp, dtype=np.float32)
    assert got.shape == exp.shape, f"{label}: shape {got.shape} != {exp.shape}"
    bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
    assert len(bad) == 0, f"{label}: {len(bad)} of {got.size} entries differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}"
