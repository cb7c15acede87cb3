"""Restatement of include/sparse_rx_facets.h in plain Python over NumPy arrays: Python ints for integer and set columns, float32
compares through NumPy for F32 columns, one binning function per mode, the live rule of tests/collapse_ref.py for lists.  It
never imports the engine."""
import bisect

import numpy as np

CODES, LABELS, EDGES = 0, 1, 2
MAX_BINS = 8192
I32, I64, F32, SET64 = 0, 1, 2, 3  # the column types of include/sparse_rx_fields.h
FITS = {CODES: (I32, I64), LABELS: (SET64,), EDGES: (I32, I64, F32)}


# ---- one binning function per mode ---------------------------------------------------------------------------------------------
def bin_codes(v: int, origin: int, n_bins: int) -> int:
    """v, origin: Python ints (nothing wraps).  The bin, or -1."""
    return v - origin if v >= origin and v - origin < n_bins else -1


def bin_edges_int(v: int, edges, n_bins: int) -> int:
    """edges: n_bins + 1 ascending Python ints.  (number of j with edges[j] <= v) - 1 when that is a bin, else -1."""
    b = bisect.bisect_right(edges, v) - 1  # ascending: the count of entries <= v
    return b if 0 <= b < n_bins else -1


def bin_edges_f32(v, edges_f32: np.ndarray, n_bins: int) -> int:
    """v: np.float32; edges_f32: float32[n_bins + 1].  IEEE compares: a NaN is below every edge (no bin), -0 == +0."""
    b = int(np.count_nonzero(edges_f32 <= np.float32(v))) - 1
    return b if 0 <= b < n_bins else -1


def label_bins(v: int, n_bins: int):
    """v: the set's 64 bits as a Python int (signed or unsigned).  The bins i < n_bins whose bit is set."""
    v &= (1 << 64) - 1
    return [i for i in range(n_bins) if (v >> i) & 1]


def edges_as_f32(edges) -> np.ndarray:
    """The float32 an int64 edge entry holds in its low 32 bits"""
    return (np.asarray(edges, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


# ---- the bins of every doc of a column -----------------------------------------------------------------------------------------
def doc_bins(col_type, data, mode, n_bins, origin=0, edges=None):
    """CODES / EDGES: int64[n_docs], the doc's bin or -1.  LABELS: bool[n_docs, n_bins]."""
    assert col_type in FITS[mode] and 1 <= n_bins <= (64 if mode == LABELS else MAX_BINS)
    n = len(data)
    if mode == LABELS:
        out = np.zeros((n, n_bins), dtype=bool)
        for d in range(n):
            out[d, label_bins(int(data[d]), n_bins)] = True
        return out
    out = np.full(n, -1, dtype=np.int64)
    if mode == CODES:
        for d in range(n):
            out[d] = bin_codes(int(data[d]), int(origin), n_bins)
    elif col_type == F32:
        e = edges_as_f32(edges)
        assert len(e) == n_bins + 1
        vals = np.asarray(data, dtype=np.float32)
        for d in range(n):
            out[d] = bin_edges_f32(vals[d], e, n_bins)
    else:
        e = [int(x) for x in edges]
        assert len(e) == n_bins + 1
        for d in range(n):
            out[d] = bin_edges_int(int(data[d]), e, n_bins)
    return out


def _count_weighted(bins, valid, weight, mode, n_bins):
    """weight: int64[n_docs], how often each doc is counted.  -> (counts int64[n_bins], (missing, other, total))"""
    has = weight if valid is None else weight * np.asarray(valid, dtype=np.int64)
    total, missing = int(weight.sum()), int((weight - has).sum())
    if mode == LABELS:
        counts = (bins.astype(np.int64) * has[:, None]).sum(axis=0)
        other = int(has[~bins.any(axis=1)].sum())
    else:
        counts = np.zeros(n_bins, dtype=np.int64)
        in_bin = bins >= 0
        np.add.at(counts, bins[in_bin], has[in_bin])
        other = int(has[~in_bin].sum())
    return counts, (missing, other, total)


def row_masks(n_docs, filter_masks, q_filter, n_rows):
    """The doc set of every output row of srx_facet_counts: filter_masks bool[n_filters, n_docs] or None (every doc); q_filter
    None (row 0) or n_rows ints, -1 = every doc."""
    out = np.ones((n_rows, n_docs), dtype=bool)
    if filter_masks is not None:
        for r in range(n_rows):
            row = 0 if q_filter is None else int(q_filter[r])
            if row >= 0:
                out[r] = np.asarray(filter_masks)[row][:n_docs]
    return out


def facet_counts(col_type, data, valid, mode, n_bins, origin=0, edges=None, filter_masks=None, q_filter=None, n_rows=1, bins=None):
    """srx_facet_counts -> (counts i32[n_rows, n_bins], extra i32[n_rows, 3]).  ``bins``: doc_bins(...) computed before, to share."""
    n_docs = len(data)
    bins = doc_bins(col_type, data, mode, n_bins, origin, edges) if bins is None else bins
    masks = row_masks(n_docs, filter_masks, q_filter, n_rows)
    counts, extra = np.zeros((n_rows, n_bins), np.int32), np.zeros((n_rows, 3), np.int32)
    for r in range(n_rows):
        counts[r], extra[r] = _count_weighted(bins, valid, masks[r].astype(np.int64), mode, n_bins)
    return counts, extra


def live_locals(n_docs, doc_base, doc, count):
    """The local docs of the LIVE positions of one list (the rule of tests/collapse_ref.py), one entry per position"""
    m = len(doc)
    live_prefix = m if count is None else min(max(int(count), 0), m)
    out = []
    for c in range(live_prefix):
        local = int(doc[c]) - int(doc_base)
        if 0 <= local < n_docs:
            out.append(local)
    return out


def facet_counts_lists(col_type, data, valid, mode, n_bins, doc_base, cand_doc, cand_count, origin=0, edges=None, bins=None):
    """srx_facet_counts_lists -> (counts i32[nq, n_bins], extra i32[nq, 3]); a doc listed twice counts twice"""
    n_docs = len(data)
    cand_doc = np.asarray(cand_doc)
    nq = cand_doc.shape[0]
    bins = doc_bins(col_type, data, mode, n_bins, origin, edges) if bins is None else bins
    counts, extra = np.zeros((nq, n_bins), np.int32), np.zeros((nq, 3), np.int32)
    for q in range(nq):
        weight = np.zeros(n_docs, dtype=np.int64)
        np.add.at(weight, np.asarray(live_locals(n_docs, doc_base, cand_doc[q], None if cand_count is None else cand_count[q]), dtype=np.int64), 1)
        counts[q], extra[q] = _count_weighted(bins, valid, weight, mode, n_bins)
    return counts, extra


def check_invariants(mode, counts, extra, bins=None):
    """CODES / EDGES: sum(bins) + missing + other == total.  LABELS: sum(bins) >= docs with a counted label = total - missing - other."""
    counts, extra = np.asarray(counts, dtype=np.int64), np.asarray(extra, dtype=np.int64)
    assert (counts >= 0).all() and (extra >= 0).all()
    if mode == LABELS:
        labelled = extra[:, 2] - extra[:, 0] - extra[:, 1]
        assert (labelled >= 0).all() and (counts.sum(axis=1) >= labelled).all() and (counts.max(axis=1) <= labelled).all()
    else:
        assert (counts.sum(axis=1) + extra[:, 0] + extra[:, 1] == extra[:, 2]).all()
