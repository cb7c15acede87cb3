"""NumPy restatement of include/sparse_rx_filter.h, written from the header: the filter row layout and what a filtered
search returns.  Shared by test_filter_cpu.py and test_filter_gpu.py; nothing here calls the engine."""
import numpy as np


def words(n_docs):
    """Words per row: ceil(n_docs / 32) rounded up to a multiple of 4."""
    return ((n_docs + 31) // 32 + 3) // 4 * 4


def pack(mask):
    """bool[n_docs] -> uint32[words(n_docs)]: doc d is allowed iff bit d & 31 of word d >> 5 is set; every other bit is 0."""
    mask = np.asarray(mask, dtype=bool)
    out = np.zeros(words(len(mask)), dtype=np.uint32)
    d = np.flatnonzero(mask)
    np.bitwise_or.at(out, d >> 5, (np.uint32(1) << (d & 31).astype(np.uint32)).astype(np.uint32))
    return out


def unpack(row, n_docs):
    """uint32 row -> bool[n_docs]; bits at or above n_docs are not docs."""
    row = np.asarray(row).view(np.uint32).reshape(-1)
    d = np.arange(n_docs)
    return ((row[d >> 5] >> (d & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def popcount(row, n_docs):
    return int(unpack(row, n_docs).sum())


def filtered_rows(full_doc, full_score, full_count, masks, doc_base, k):
    """The rows a filtered search returns, from the UNFILTERED ranking at unlimited depth (full_doc i32[nq, K] GLOBAL ids,
    full_score f32[nq, K], full_count i32[nq]; K >= every count): the rows of disallowed docs removed, cut to k, padded with
    -1 / +0.0.  masks: one bool[n_docs] over LOCAL rows for all queries, or a sequence of nq masks where None means "this
    query is not filtered"."""
    nq = len(full_count)
    per_query = isinstance(masks, (list, tuple))
    out_d = np.full((nq, k), -1, np.int32)
    out_s = np.zeros((nq, k), np.float32)
    out_c = np.zeros(nq, np.int32)
    for q in range(nq):
        c = int(full_count[q])
        d, s = full_doc[q, :c], full_score[q, :c]
        m = masks[q] if per_query else masks
        if m is not None:
            keep = np.asarray(m, dtype=bool)[d.astype(np.int64) - doc_base]
            d, s = d[keep], s[keep]
        n = min(k, len(d))
        out_d[q, :n], out_s[q, :n], out_c[q] = d[:n], s[:n], n
    return out_d, out_s, out_c
