"""NumPy restatement of include/asym/sparse_rx_binary_asym.h, written from its stated contract: the 4-bit query codes, the integer
score against 1-bit rows, the (score descending, doc ascending) top-m under a filter and the scores of given docs.  The bits, the
filter rows and the cut of a screened search come from tests/binary_ref.py.  Nothing here imports the package."""
import numpy as np

import binary_ref as bref

INT32_MIN = -2 ** 31


def quantize(q, center=None, dim_pad=None):
    """f32[nq, dim] -> i8[nq, dim_pad]: every step one fp32 operation, as the header lists them"""
    q = np.asarray(q, dtype=np.float32)
    nq, dim = q.shape
    dim_pad = bref.pad128(dim) if dim_pad is None else int(dim_pad)
    with np.errstate(all="ignore"):
        r = q if center is None else (q - np.asarray(center, np.float32)[None, :]).astype(np.float32)
        mag = np.abs(r)
        amax = np.where(np.isnan(mag), np.float32(0), mag).max(axis=1).astype(np.float32)
        inv = np.where(amax > 0, np.float32(7) / amax, np.float32(0)).astype(np.float32)
        p = (r * inv[:, None]).astype(np.float32)
        c = np.clip(np.rint(p), -7, 7)  # np.rint: to nearest even
        c[np.isnan(p)] = 0
    codes = np.zeros((nq, dim_pad), np.int8)
    codes[:, :dim] = c.astype(np.int8)
    return codes


def scores(codes, d_bits):
    """i8[nq, dim_pad], u32[n, W] -> i64[nq, n]: sum code * (2 bit - 1)"""
    bits = np.unpackbits(np.ascontiguousarray(d_bits).view(np.uint8), axis=1, bitorder="little").astype(np.int64)
    return np.asarray(codes, np.int64) @ (2 * bits - 1).T


def search(codes, d_bits, m, doc_base=0, masks=None, q_filter=None):
    """-> (doc i32[nq, m], score i32[nq, m], count i32[nq]): lexsort((doc, -score)) under the mask, padding -1 / INT32_MIN"""
    nq, n = codes.shape[0], d_bits.shape[0]
    s = scores(codes, d_bits)
    allow = bref.filter_masks(masks, q_filter, nq, n)
    doc = np.full((nq, m), -1, np.int32)
    out = np.full((nq, m), INT32_MIN, np.int32)
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        ids = np.flatnonzero(allow[q])
        order = ids[np.lexsort((ids, -s[q, ids]))][:m]
        cnt[q] = len(order)
        doc[q, : len(order)] = order + doc_base
        out[q, : len(order)] = s[q, order]
    return doc, out, cnt


def score_docs(codes, d_bits, cand_doc, cand_count=None, doc_base=0):
    """i32[nq, m]: scores of the given GLOBAL ids; padding and ids outside the shard give INT32_MIN"""
    cand_doc = np.asarray(cand_doc)
    nq, m = cand_doc.shape
    s = scores(codes, d_bits)
    local = cand_doc.astype(np.int64) - doc_base
    lim = np.full(nq, m) if cand_count is None else np.clip(np.asarray(cand_count), 0, m)
    ok = (local >= 0) & (local < d_bits.shape[0]) & (np.arange(m)[None, :] < lim[:, None])
    return np.where(ok, np.take_along_axis(s, np.where(ok, local, 0), axis=1), INT32_MIN).astype(np.int32)
