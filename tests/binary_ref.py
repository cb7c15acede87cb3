"""NumPy restatement of include/binary/sparse_rx_binary.h and of the screened search of sparse_rx/binary.py, written from their
stated contracts: codes, the tiled layout, Hamming distances, the (distance ascending, doc ascending) top-m under a filter,
and the pool -> exact scores -> cut of ``ScreenedDenseIndex``.  Nothing here imports the package."""
import numpy as np

MAX_K = 1024
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)  # byte popcount table


def pad128(dim):
    return (int(dim) + 127) // 128 * 128


def encode(x, center=None, dim_pad=None):
    """f32[n, dim] -> u32[n, dim_pad / 32]: bit c = x[c] > center[c] as an fp32 compare (NaN, -0.0, equality: 0), column c is
    bit c & 31 of word c >> 5, bits at or above dim are 0."""
    x = np.asarray(x, dtype=np.float32)
    n, dim = x.shape
    dim_pad = pad128(dim) if dim_pad is None else int(dim_pad)
    c = np.zeros(dim, np.float32) if center is None else np.asarray(center, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        b = np.zeros((n, dim_pad), dtype=bool)
        b[:, :dim] = x > c[None, :]
    return np.packbits(b, axis=1, bitorder="little").view("<u4").reshape(n, dim_pad // 32)


def tiled_index(r, w, W):
    """u32 index of word w of row r in the tiled corpus"""
    return (((r >> 6) * (W // 4) + (w >> 2)) * 64 + (r & 63)) * 4 + (w & 3)


def tile(bits):
    """u32[n, W] -> the tiled buffer u32[ceil(n / 64) * 64 * W]; rows past n are zeros"""
    n, W = bits.shape
    out = np.zeros(-(-n // 64) * 64 * W, dtype=np.uint32)
    r, w = np.meshgrid(np.arange(n), np.arange(W), indexing="ij")
    out[tiled_index(r, w, W)] = bits
    return out


def untile(buf, n, W):
    r, w = np.meshgrid(np.arange(n), np.arange(W), indexing="ij")
    return np.asarray(buf).view(np.uint32)[tiled_index(r, w, W)]


def distances(q_bits, d_bits):
    """u32[nq, W], u32[n, W] -> i32[nq, n]"""
    q8 = np.ascontiguousarray(q_bits).view(np.uint8)
    d8 = np.ascontiguousarray(d_bits).view(np.uint8)
    out = np.empty((q8.shape[0], d8.shape[0]), dtype=np.int32)
    for i in range(q8.shape[0]):
        out[i] = _POP8[q8[i][None, :] ^ d8].sum(axis=1)
    return out


def filter_masks(filter_masks_, q_filter, nq, n):
    """bool[nq, n]: the docs each query may return (q_filter None: row 0 for all; -1: not filtered)"""
    if filter_masks_ is None:
        return np.ones((nq, n), dtype=bool)
    fm = np.asarray(filter_masks_, dtype=bool).reshape(-1, n)
    rows = np.zeros(nq, np.int64) if q_filter is None else np.asarray(q_filter)
    return np.stack([np.ones(n, dtype=bool) if r < 0 else fm[r] for r in rows]) if nq else np.ones((0, n), dtype=bool)


def search(q_bits, d_bits, m, doc_base=0, masks=None, q_filter=None):
    """-> (doc i32[nq, m], dist i32[nq, m], count i32[nq]): lexsort((doc, dist)) under the mask, padding -1 / -1"""
    nq, n = q_bits.shape[0], d_bits.shape[0]
    dist = distances(q_bits, d_bits)
    allow = filter_masks(masks, q_filter, nq, n)
    doc = np.full((nq, m), -1, np.int32)
    out = np.full((nq, m), -1, np.int32)
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        ids = np.flatnonzero(allow[q])
        order = ids[np.lexsort((ids, dist[q, ids]))][:m]
        cnt[q] = len(order)
        doc[q, : len(order)] = order + doc_base
        out[q, : len(order)] = dist[q, order]
    return doc, out, cnt


def dist_docs(q_bits, d_bits, cand_doc, cand_count=None, doc_base=0):
    """i32[nq, m]: distances of the given GLOBAL ids; padding and ids outside the shard give -1"""
    cand_doc = np.asarray(cand_doc)
    nq, m = cand_doc.shape
    n = d_bits.shape[0]
    dist = distances(q_bits, d_bits)
    out = np.full((nq, m), -1, np.int32)
    for q in range(nq):
        lim = m if cand_count is None else min(m, max(int(cand_count[q]), 0))
        for i in range(lim):
            r = int(cand_doc[q, i]) - doc_base
            if 0 <= r < n:
                out[q, i] = dist[q, r]
    return out


def screen_pool(k, oversample, n_docs):
    return min(max(k, k * oversample), MAX_K, n_docs)


def cut(pool_doc, pool_score, pool_count, k, score_offset=0.0):
    """The pool (docs, the exact index's scores of them, counts) -> the screened search's rows: fl32(score + offset), > 0 only,
    lexsort((doc, -score)), the best k, padding -1 / +0.0"""
    nq = pool_doc.shape[0]
    doc = np.full((nq, k), -1, np.int32)
    score = np.zeros((nq, k), np.float32)
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        c = int(pool_count[q])
        d = np.asarray(pool_doc[q, :c])
        s = (np.asarray(pool_score[q, :c], dtype=np.float32) + np.float32(score_offset)).astype(np.float32)
        keep = s > 0
        d, s = d[keep], s[keep]
        order = np.lexsort((d, -s.astype(np.float64)))[:k]
        cnt[q] = len(order)
        doc[q, : len(order)] = d[order]
        score[q, : len(order)] = s[order]
    return doc, score, cnt
