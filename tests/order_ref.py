"""NumPy / plain-Python restatement of include/order/sparse_rx_order.h, written from the header's contract and never from the
kernel: the order is a ``sorted()`` with an explicit key tuple over the row's doc set, the cursor is "keep what c precedes".
Shared by tests/test_order_cpu.py and tests/test_order_gpu.py."""
import numpy as np

ASC, DESC = 0, 1
NULLS_LAST, NULLS_FIRST, NULLS_DROP = 0, 1, 2
MAX_M, MAX_K = 2048, 1024
I32, I64, F32, SET64 = 0, 1, 2, 3
MIN_SEG, CHUNK = 32768, 8192  # the workspace formula of the header
DTYPE = {I32: np.int32, I64: np.int64, F32: np.float32}


def plan(n_docs, n_rows, k):
    """(segments, workspace bytes) by the header's formula"""
    seg_docs = CHUNK * ((max(MIN_SEG, 64 * k) + CHUNK - 1) // CHUNK)
    segments = (n_docs + seg_docs - 1) // seg_docs
    return segments, n_rows * segments * (12 * k + 8)


def has_value(col_type, data, valid):
    """bool[n_docs]: the valid bit is set (or there is no validity row) and, for F32, the value is not NaN"""
    has = np.ones(len(data), dtype=bool) if valid is None else np.asarray(valid, dtype=bool).copy()
    if col_type == F32:
        has &= ~np.isnan(np.asarray(data, dtype=np.float32))
    return has


def raw_key(col_type, data, d):
    """out_key of a doc that has a value: the value as int64; F32: the stored bits in the low 32, zero-extended"""
    if col_type == F32:
        return int(np.asarray(data, dtype=np.float32)[d: d + 1].view(np.uint32)[0])
    return int(data[d])


def doc_keys(col_type, data, valid, order, nulls):
    """(has bool[n_docs], key: one tuple per doc) -- doc a precedes doc b iff key[a] < key[b].  The tuple is (class, value or its
    negative under DESC, doc): Python compares ints of any size exactly and floats by IEEE with -0.0 == 0.0."""
    has = has_value(col_type, data, valid)
    first = nulls == NULLS_FIRST
    vals = np.asarray(data, dtype=DTYPE[col_type]).tolist()
    keys = []
    for d, (h, v) in enumerate(zip(has.tolist(), vals)):
        if h:
            keys.append((1 if first else 0, v if order == ASC else -v, d))
        else:
            keys.append((0 if first else 1, 0, d))
    return has, keys


def order_topk(col_type, data, valid, doc_base, order, nulls, k, masks=None, q_filter=None, n_rows=1, after=None, keys=None):
    """srx_order_topk: (out_doc i32[n_rows, k], out_key i64[n_rows, k], out_extra i32[n_rows, 3]).  masks: bool[n_filters, >= n_docs]
    or None (a NULL filter); q_filter / after: sequences or None."""
    n = len(data)
    has, key = keys if keys is not None else doc_keys(col_type, data, valid, order, nulls)
    out_doc = np.full((n_rows, k), -1, dtype=np.int32)
    out_key = np.zeros((n_rows, k), dtype=np.int64)
    extra = np.zeros((n_rows, 3), dtype=np.int32)
    for r in range(n_rows):
        pick = -1 if masks is None else 0 if q_filter is None else int(q_filter[r])
        docs = list(range(n)) if pick < 0 else np.flatnonzero(np.asarray(masks[pick])[:n]).tolist()
        total = len(docs)
        if nulls == NULLS_DROP:
            docs = [d for d in docs if has[d]]
        c = -1 if after is None else int(after[r])
        if c != -1:
            lc = c - doc_base
            if not 0 <= lc < n or (nulls == NULLS_DROP and not has[lc]):
                docs = []
            else:
                docs = [d for d in docs if key[lc] < key[d]]  # c strictly precedes d
        ranked = sorted(docs, key=key.__getitem__)[:k]
        for i, d in enumerate(ranked):
            out_doc[r, i] = doc_base + d
            out_key[r, i] = raw_key(col_type, data, d) if has[d] else 0
        extra[r] = (len(ranked), sum(1 for d in ranked if has[d]), total)
    return out_doc, out_key, extra


def order_lists(col_type, data, valid, doc_base, order, nulls, cand_doc, cand_score, cand_count, k):
    """srx_order_lists: (out_doc i32[nq, k], out_score as uint32 bits [nq, k], out_key i64[nq, k], out_pos i32[nq, k],
    out_extra i32[nq, 3])"""
    n = len(data)
    has, key = doc_keys(col_type, data, valid, order, nulls)
    cand_doc = np.asarray(cand_doc)
    bits = np.ascontiguousarray(cand_score, dtype=np.float32).view(np.uint32)
    nq, m = cand_doc.shape
    out_doc = np.full((nq, k), -1, dtype=np.int32)
    out_bits = np.zeros((nq, k), dtype=np.uint32)
    out_key = np.zeros((nq, k), dtype=np.int64)
    out_pos = np.full((nq, k), -1, dtype=np.int32)
    extra = np.zeros((nq, 3), dtype=np.int32)
    for q in range(nq):
        n_live = m if cand_count is None else min(max(int(cand_count[q]), 0), m)
        live = [c for c in range(n_live) if 0 <= int(cand_doc[q, c]) - doc_base < n]
        local = {c: int(cand_doc[q, c]) - doc_base for c in live}
        kept = [c for c in live if has[local[c]] or nulls != NULLS_DROP]
        ranked = sorted(kept, key=lambda c: key[local[c]][:2] + (c,))[:k]  # the tie-break is the position, not the doc
        for i, c in enumerate(ranked):
            out_doc[q, i], out_bits[q, i], out_pos[q, i] = cand_doc[q, c], bits[q, c], c
            out_key[q, i] = raw_key(col_type, data, local[c]) if has[local[c]] else 0
        extra[q] = (len(ranked), sum(1 for c in ranked if has[local[c]]), len(live))
    return out_doc, out_bits, out_key, out_pos, extra
