"""Order by a field on the GPU (include/order/sparse_rx_order.h).  Expected results are never the engine's own: the restatement
(tests/order_ref.py) over the column, the masks, the cursors and the lists a call was given.  Every comparison is exact -- doc
ids, key bits, extras, score bits, positions -- and every output buffer and the workspace are pre-filled with 0x7F7F7F7F so that a
word the call does not write shows.

The kernel's sizes (csrc/order.hip): a workgroup scans a segment of max(32 768, 64 k) docs (whole 8 192-doc chunks) for one row,
appends to a list of 2 048 ranks (k <= 512; 4 096 above) and cuts it to k whenever more than half of it is held;
``_capi.order_plan`` tells the segments."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import order_ref  # noqa: E402
from order_ref import ASC, DESC, F32, I32, I64, NULLS_DROP, NULLS_FIRST, NULLS_LAST  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -(2 ** 31), 2 ** 31 - 1, -(2 ** 63), 2 ** 63 - 1
GARBAGE = 0x7F7F7F7F
SEG = 32768  # a segment's docs at k <= 512
ORDERS, NULLS = (ASC, DESC), (NULLS_LAST, NULLS_FIRST, NULLS_DROP)


def _garbage(torch, shape, dtype):
    return torch.full(shape, GARBAGE, dtype=torch.int32, device=DEVICE) if dtype == torch.int32 else \
        torch.full(shape, GARBAGE * (2 ** 32 + 1), dtype=torch.int64, device=DEVICE)


class _Col:
    """One column on the device, as the C calls take it, next to its host arrays"""

    def __init__(self, col_type, data, valid=None, doc_base=0):
        import torch
        from sparse_rx import _capi
        from sparse_rx.filter import pack_masks
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.type, self.data = col_type, np.ascontiguousarray(data, dtype=order_ref.DTYPE[col_type])
        self.valid = None if valid is None else np.asarray(valid, dtype=bool)
        self.n_docs, self.doc_base = len(self.data), doc_base
        self.data_t = torch.from_numpy(self.data).to(DEVICE)
        self.valid_t = None if valid is None else torch.from_numpy(pack_masks(self.valid).view(np.int32).copy()).to(DEVICE).reshape(-1)
        self.desc = _capi.FieldColDesc(data=self.data_t.data_ptr(), valid=None if valid is None else self.valid_t.data_ptr(), type=col_type)
        self._keys = {}

    def keys(self, order, nulls):
        if (order, nulls) not in self._keys:
            self._keys[order, nulls] = order_ref.doc_keys(self.type, self.data, self.valid, order, nulls)
        return self._keys[order, nulls]

    def topk(self, order, nulls, k, masks=None, q_filter=None, n_rows=1, after=None, bits=None, stream=None, bufs=None, label=""):
        """srx_order_topk on garbage-filled outputs and workspace against the restatement.  masks: bool[n_filters, n_docs] or None
        (a NULL filter); bits: the packed rows to upload in place of pack_masks(masks)."""
        import ctypes
        import torch
        from sparse_rx import _capi
        from sparse_rx.filter import pack_masks
        fdesc = keep = None
        if masks is not None:
            packed = pack_masks(np.asarray(masks, dtype=bool)) if bits is None else bits
            bits_t = torch.from_numpy(packed.view(np.int32).copy()).to(DEVICE)
            q_t = None if q_filter is None else torch.from_numpy(np.ascontiguousarray(q_filter, dtype=np.int32)).to(DEVICE)
            keep = _capi.DocFilterDesc(bits=bits_t.data_ptr(), n_filters=int(bits_t.shape[0]), q_filter=None if q_t is None else q_t.data_ptr())
            fdesc = ctypes.byref(keep)
        a_t = None if after is None else torch.from_numpy(np.ascontiguousarray(after, dtype=np.int32)).to(DEVICE)
        ws_bytes = _capi.order_plan(self.n_docs, n_rows, k)[1]
        if bufs is None:
            bufs = (_garbage(torch, (n_rows, k), torch.int32), _garbage(torch, (n_rows, k), torch.int64), _garbage(torch, (n_rows, 3), torch.int32))
        ws = _garbage(torch, ((ws_bytes + 7) // 8,), torch.int64)
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        rc = _capi.lib().srx_order_topk(0, ctypes.byref(self.desc), self.n_docs, self.doc_base, order, nulls, fdesc, n_rows, k,
                                        None if a_t is None else a_t.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                        ws.data_ptr(), ws_bytes, sp)
        _capi.check(rc, "srx_order_topk")
        torch.cuda.synchronize()
        doc, key, extra = (t.cpu().numpy() for t in bufs)
        ed, ek, ee = order_ref.order_topk(self.type, self.data, self.valid, self.doc_base, order, nulls, k, masks, q_filter, n_rows, after,
                                          keys=self.keys(order, nulls))
        where = (label, order, nulls, k)
        assert np.array_equal(extra, ee), (where, "extra", extra[:6], ee[:6])
        assert np.array_equal(doc, ed), (where, "doc", np.argwhere(doc != ed)[:6])
        assert np.array_equal(key, ek), (where, "key", np.argwhere(key != ek)[:6])
        return doc, key, extra, bufs

    def lists(self, order, nulls, k, doc, score, count, want_pos=True, stream=None, label=""):
        import ctypes
        import torch
        from sparse_rx import _capi
        doc = np.ascontiguousarray(doc, dtype=np.int32)
        score = np.ascontiguousarray(score, dtype=np.float32)
        nq, m = doc.shape
        d_t, s_t = torch.from_numpy(doc).to(DEVICE), torch.from_numpy(score.view(np.int32)).to(DEVICE)
        c_t = None if count is None else torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).to(DEVICE)
        outs = [_garbage(torch, (nq, k), torch.int32), _garbage(torch, (nq, k), torch.int32), _garbage(torch, (nq, k), torch.int64),
                _garbage(torch, (nq, k), torch.int32), _garbage(torch, (nq, 3), torch.int32)]
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        rc = _capi.lib().srx_order_lists(0, ctypes.byref(self.desc), self.n_docs, self.doc_base, order, nulls, d_t.data_ptr(), s_t.data_ptr(),
                                         None if c_t is None else c_t.data_ptr(), nq, m, k, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                         outs[3].data_ptr() if want_pos else None, outs[4].data_ptr(), sp)
        _capi.check(rc, "srx_order_lists")
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in outs]
        want = order_ref.order_lists(self.type, self.data, self.valid, self.doc_base, order, nulls, doc, score, count, k)
        where = (label, order, nulls, k, m)
        assert np.array_equal(got[4], want[4]), (where, "extra", got[4][:6], want[4][:6])
        assert np.array_equal(got[0], want[0]), (where, "doc", np.argwhere(got[0] != want[0])[:6])
        assert np.array_equal(got[1].view(np.uint32), want[1]), (where, "score bits")
        assert np.array_equal(got[2], want[2]), (where, "key")
        if want_pos:
            assert np.array_equal(got[3], want[3]), (where, "pos")
        else:
            assert (got[3] == GARBAGE).all()  # a NULL out_pos: nothing is written for it
        return got


def _masks(rng, n_docs, densities=(0.5, 1.0, 2.0 ** -10, 0.0, 0.05)):
    m = np.zeros((len(densities), n_docs), dtype=bool)
    for i, p in enumerate(densities):
        m[i] = rng.random(n_docs) < p
    if n_docs > 1:
        m[0, 0], m[0, -1] = True, True
    return m


def _column(col_type, n_docs, rng, distinct=None):
    if col_type == F32:
        return (rng.integers(-50, 50, n_docs) / 4).astype(np.float32) if distinct is None else rng.integers(0, distinct, n_docs).astype(np.float32)
    span = 2 ** 40 if col_type == I64 else 1000
    return rng.integers(-span, span, n_docs) if distinct is None else rng.integers(0, distinct, n_docs)


Q_FILTER = [0, 1, 2, 3, 4, 0, -1, 2, 0]  # five rows, with repeats and -1


# ---- 1. the base shape: every type, order, nulls mode, with and without a validity row -----------------------------------------
@pytest.mark.parametrize("col_type", [I32, I64, F32])
def test_base_shape(col_type):
    from sparse_rx import _capi
    n_docs = 3000
    assert _capi.order_plan(n_docs, 9, 64)[0] == 1  # one segment
    rng = np.random.default_rng(10 + col_type)
    masks = _masks(rng, n_docs)
    for valid in (None, rng.random(n_docs) > 0.3):
        col = _Col(col_type, _column(col_type, n_docs, rng), valid, doc_base=1000)
        for order in ORDERS:
            for nulls in NULLS:
                col.topk(order, nulls, 64, masks, Q_FILTER, len(Q_FILTER), label=f"type {col_type}")
        col.topk(DESC, NULLS_LAST, 7, masks, None, 3, label="a NULL q_filter: row 0 three times")
        col.topk(ASC, NULLS_FIRST, 7, None, None, 2, label="a NULL filter: every doc")


@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 127, 128, 129, SEG - 1, SEG, SEG + 1])
def test_geometry(n_docs):
    from sparse_rx import _capi
    assert _capi.order_plan(n_docs, 1, 7)[0] == (2 if n_docs > SEG else 1)
    rng = np.random.default_rng(n_docs)
    valid = rng.random(n_docs) > 0.2
    valid[[0, -1]] = False
    col = _Col(I32, _column(I32, n_docs, rng, distinct=5), valid, doc_base=7)
    masks = _masks(rng, n_docs)
    for nulls in NULLS:
        col.topk(DESC, nulls, 7, masks, [0, 1, 2, 3, -1], 5)
        col.topk(ASC, nulls, 1, masks, [-1, 0], 2)


@pytest.mark.parametrize("k", [1, 7, 64, 1000, 1024])
def test_several_segments_and_every_k(k):
    """200 000 int32 docs: 7 segments at k <= 512 and 4 at 1 000 / 1 024; rows dense, full, sparse (2^-10: fewer docs than k =
    1 000), empty and through -1; five distinct values, so ties fall at every cut"""
    from sparse_rx import _capi
    n_docs = 200000
    assert _capi.order_plan(n_docs, 1, k)[0] == (7 if k <= 512 else 4) >= 3
    rng = np.random.default_rng(k)
    masks = _masks(rng, n_docs)
    assert 0 < masks[2].sum() < 1000 and masks[3].sum() == 0
    valid = rng.random(n_docs) > 0.01
    col = _Col(I32, _column(I32, n_docs, rng, distinct=5), valid)
    col.topk(DESC, NULLS_LAST, k, masks, [0, 2, 3, -1], 4, label="five values")
    col.topk(ASC, NULLS_FIRST, k, masks, [2, 1], 2, label="five values")
    wide = _Col(I64, _column(I64, n_docs, rng), None, doc_base=12345)
    wide.topk(ASC, NULLS_DROP, k, masks, [0, 2], 2, label="distinct values")


def test_every_doc_beats_the_threshold():
    """An ascending column read newest first, and an all-equal one: every doc of a segment enters the list, which is cut again
    and again"""
    n_docs = 100000
    masks = _masks(np.random.default_rng(3), n_docs, (0.9, 1.0))
    for k in (10, 1000):
        _Col(I64, np.arange(n_docs) * 3 - 7, None).topk(DESC, NULLS_LAST, k, masks, [0, -1], 2, label="ascending column")
        _Col(I32, np.full(n_docs, 42), None).topk(DESC, NULLS_LAST, k, masks, [0, 1], 2, label="all equal")
        _Col(I32, np.full(n_docs, 42), np.zeros(n_docs, dtype=bool)).topk(ASC, NULLS_FIRST, k, masks, [0], 1, label="no doc has a value")


def test_extremes():
    rng = np.random.default_rng(5)
    n_docs = 500
    for col_type, lo, hi in ((I32, I32_MIN, I32_MAX), (I64, I64_MIN, I64_MAX)):
        pool = np.array([lo, lo + 1, -1, 0, 1, hi - 1, hi, 2 ** 31 if col_type == I64 else 7, -(2 ** 32) if col_type == I64 else -7], dtype=order_ref.DTYPE[col_type])
        col = _Col(col_type, pool[rng.integers(0, len(pool), n_docs)], rng.random(n_docs) > 0.1)
        for order in ORDERS:
            for nulls in NULLS:
                col.topk(order, nulls, 64, None, None, 1, label="extremes")
                col.topk(order, nulls, n_docs, None, None, 1, label="extremes, all")
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 3.4028235e38, -3.4028235e38, 1.0, -1.0],
                        dtype=np.float32)
    bits = specials.view(np.uint32).copy()
    bits = np.concatenate([bits, np.array([0xFFC00001, 0x7F800001], dtype=np.uint32)])  # two more NaN encodings
    data = bits[rng.integers(0, len(bits), n_docs)].view(np.float32)
    for valid in (None, rng.random(n_docs) > 0.1):
        col = _Col(F32, data, valid, doc_base=3)
        for order in ORDERS:
            for nulls in NULLS:
                doc, key, extra, _ = col.topk(order, nulls, n_docs, None, None, 1, label="float specials")
        assert (key == 0x80000000).any()  # -0 keeps its bits in out_key


def test_valueless_docs_straddle_k():
    n_docs = 300
    rng = np.random.default_rng(8)
    valid = np.zeros(n_docs, dtype=bool)
    valid[rng.choice(n_docs, 10, replace=False)] = True
    col = _Col(I64, _column(I64, n_docs, rng), valid)
    mask = np.zeros((1, n_docs), dtype=bool)
    mask[0, rng.choice(n_docs, 40, replace=False)] = True
    mask[0, valid] = True
    for k in (7, 9, 10, 11, 13, 64):
        for nulls in NULLS:
            col.topk(DESC, nulls, k, mask, [0], 1, label="ten valued docs")


@pytest.mark.parametrize("n_docs", [1, 33, 100, 2049, SEG + 5])
def test_bits_at_or_above_n_docs_do_not_belong(n_docs):
    from sparse_rx.filter import pack_masks
    rng = np.random.default_rng(n_docs)
    col = _Col(I32, _column(I32, n_docs, rng, distinct=4))
    masks = _masks(rng, n_docs, (0.5, 0.0))
    bits = pack_masks(masks).copy()
    bits |= ~pack_masks(np.ones((2, n_docs), dtype=bool))  # the tail of the last word and the padding words
    assert (bits[:, -1] != 0).all() or n_docs % 128 == 0
    col.topk(ASC, NULLS_LAST, 64, masks, [0, 1], 2, bits=bits)


# ---- 2. the cursor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", NULLS)
def test_pages_of_seven_reproduce_the_order(nulls):
    n_docs, base = 40000, 500  # two segments
    rng = np.random.default_rng(20 + nulls)
    col = _Col(I32, _column(I32, n_docs, rng, distinct=9), rng.random(n_docs) > 0.3, doc_base=base)
    masks = _masks(rng, n_docs, (0.006, 0.005))
    whole = [order_ref.order_topk(I32, col.data, col.valid, base, DESC, nulls, n_docs, masks, [r], 1, keys=col.keys(DESC, nulls)) for r in (0, 1)]
    want = [w[0][0, : w[2][0, 0]].tolist() for w in whole]
    assert all(100 < len(w) < 300 for w in want)
    got, after, live = [[], []], [-1, -1], True
    pages = 0
    while live:
        doc, _, extra, _ = col.topk(DESC, nulls, 7, masks, [0, 1], 2, after=after, label=f"page {pages}")
        for r in (0, 1):
            got[r] += doc[r, : extra[r, 0]].tolist()
            after[r] = got[r][-1] if got[r] else -1
        live = bool((extra[:, 0] == 7).any())
        pages += 1
        assert pages < 60
    assert got == want


def test_cursors():
    n_docs, base = 3000, 1000
    rng = np.random.default_rng(31)
    valid = rng.random(n_docs) > 0.3
    col = _Col(F32, _column(F32, n_docs, rng), valid, doc_base=base)
    masks = _masks(rng, n_docs)
    outside_set = int(np.flatnonzero(~masks[0] & valid)[0]) + base
    valueless = int(np.flatnonzero(~valid)[0]) + base
    after = [outside_set, valueless, -1, base - 1, base + n_docs, -2, I32_MAX, base, base + n_docs - 1]
    for order in ORDERS:
        for nulls in NULLS:
            doc, key, extra, _ = col.topk(order, nulls, 64, masks, [0] * len(after), len(after), after=after, label="cursors")
            assert (extra[:, 2] == masks[0].sum()).all()                  # total is intact whatever the cursor
            assert (extra[3:7, 0] == 0).all() and (doc[3:7] == -1).all()  # an id outside the index: empty
            assert (extra[1, 0] == 0) == (nulls == NULLS_DROP)            # a valueless cursor: empty under DROP only
    assert col.topk(ASC, NULLS_DROP, 64, masks, [0, -1], 2, after=[valueless, valueless])[2][:, 0].tolist() == [0, 0]
    col.topk(ASC, NULLS_LAST, 64, None, None, 2, after=[outside_set, -1], label="cursor without a filter")


# ---- 3. execution ------------------------------------------------------------------------------------------------------------------
def test_side_stream_and_second_call():
    import torch
    n_docs = 2 * SEG + 5
    rng = np.random.default_rng(77)
    col = _Col(I64, _column(I64, n_docs, rng), rng.random(n_docs) > 0.1)
    masks = _masks(rng, n_docs)
    side = torch.cuda.Stream(device=DEVICE)
    d1, k1, e1, bufs = col.topk(DESC, NULLS_LAST, 64, masks, [0, 1, 2, 3], 4, stream=side)
    d2, k2, e2, _ = col.topk(DESC, NULLS_LAST, 64, masks, [0, 1, 2, 3], 4, bufs=bufs)  # into the buffers that hold a result
    assert np.array_equal(d1, d2) and np.array_equal(k1, k2) and np.array_equal(e1, e2)
    col.topk(ASC, NULLS_DROP, 64, masks, [3, 2, 1, 0], 4, bufs=bufs)                    # and another result over them
    lists = rng.integers(0, n_docs, (4, 700))
    col.lists(DESC, NULLS_LAST, 700, lists, rng.random((4, 700)), None, stream=side)


def test_more_rows_than_the_grid_has():
    n_docs, n_rows = 33, 65535 + 4
    rng = np.random.default_rng(9)
    col = _Col(I32, _column(I32, n_docs, rng, distinct=3), rng.random(n_docs) > 0.2)
    col.topk(DESC, NULLS_LAST, 1, _masks(rng, n_docs, (0.5, 1.0, 0.1)), rng.integers(-1, 3, n_rows), n_rows, after=rng.integers(-1, n_docs, n_rows))


# ---- 4. lists ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 64, 2048])
def test_lists(m):
    n_docs, base, nq = 5000, 100, 9
    rng = np.random.default_rng(m)
    valid = rng.random(n_docs) > 0.25
    doc = rng.integers(base - 20, base + n_docs + 20, (nq, m))  # some ids outside the index on both sides
    doc[0, :] = doc[0, 0]                                        # one doc m times
    doc[1, m // 2:] = doc[1, : m - m // 2]                       # every doc twice
    score = rng.standard_normal((nq, m)).astype(np.float32)     # negative scores too
    score[2, :: 3] = np.nan
    score.view(np.uint32)[3, 0] = 0xFFC12345                     # a NaN payload travels bit for bit
    count = np.array([m, m, 0, -5, m + 3, m // 2, 1, m, max(m - 1, 0)], dtype=np.int32)
    for col_type, distinct in ((I32, 4), (I64, None), (F32, 6)):  # few values: ties keep list order
        col = _Col(col_type, _column(col_type, n_docs, rng, distinct), valid, doc_base=base)
        for order in ORDERS:
            for nulls in NULLS:
                for k in sorted({1, (m + 1) // 2, m}):
                    col.lists(order, nulls, k, doc, score, count, label="lists")
        col.lists(DESC, NULLS_LAST, m, doc, score, None, label="a NULL cand_count")
        col.lists(ASC, NULLS_FIRST, m, doc, score, count, want_pos=False, label="a NULL out_pos")


def test_lists_nulls_at_the_cut():
    n_docs, m = 200, 40
    rng = np.random.default_rng(2)
    valid = np.zeros(n_docs, dtype=bool)
    valid[:100] = True
    col = _Col(I32, _column(I32, n_docs, rng, distinct=3), valid)
    doc = np.stack([rng.permutation(np.concatenate([rng.choice(100, 10, replace=False), 100 + rng.choice(100, 30, replace=False)])) for _ in range(3)])
    for k in (9, 10, 11, 30, 31, 40):
        for nulls in NULLS:
            col.lists(DESC, nulls, k, doc, rng.random((3, m)), None, label="ten valued positions")


def test_field_table_host_doors_at_the_smallest_shape():
    """``FieldTable.sort_lists`` and ``top_by`` with a host ``q_filter``: host arrays in and out over a 70-doc table with a
    doc_base, whose validity row ends in a partial word; nq = 2, m = 3, k = 2."""
    from sparse_rx.fields import FieldTable
    from sparse_rx.filter import DocFilter
    n_docs, base = 70, 1000
    rng = np.random.default_rng(70)
    values, missing = rng.integers(-5, 5, n_docs).astype(np.int64), np.arange(n_docs) % 7 == 6  # doc 69 has no value
    valid = ~missing
    table = FieldTable.from_columns({"stamp": np.ma.array(values, mask=missing)}, device=DEVICE, doc_base=base)
    doc = np.array([[base + 69, base + 3, base + 64], [base + 5, base - 1, base + 68]], dtype=np.int32)  # one id outside the table
    score = np.array([[3.0, 2.0, 1.0], [0.5, -1.0, np.nan]], dtype=np.float32)
    for count in (None, np.array([3, 2], dtype=np.int32)):
        for order, o in (("asc", ASC), ("desc", DESC)):
            for nulls, nl in (("last", NULLS_LAST), ("first", NULLS_FIRST), ("drop", NULLS_DROP)):
                got = table.sort_lists("stamp", doc, score, count, 2, order=order, nulls=nulls, want_pos=True)
                ed, es, ek, ep, ee = order_ref.order_lists(I64, values, valid, base, o, nl, doc, score, count, 2)
                assert all(isinstance(a, np.ndarray) for a in got) and len(got) == 5
                assert np.array_equal(got[0], ed) and np.array_equal(got[1].view(np.uint32), es) and np.array_equal(got[2], ek), (order, nulls)
                assert np.array_equal(got[3], ee) and np.array_equal(got[4], ep), (order, nulls)
    masks = np.zeros((2, n_docs), dtype=bool)
    masks[0, ::2], masks[1, 60:] = True, True
    flt = DocFilter.from_masks(masks, device=DEVICE, doc_base=base)
    got_doc, got_key, has, extra = table.top_by("stamp", 2, order="asc", nulls="last", filter=flt, q_filter=[1, -1, 0])
    ed, ek, ee = order_ref.order_topk(I64, values, valid, base, ASC, NULLS_LAST, 2, masks, [1, -1, 0], 3)
    assert np.array_equal(got_doc, ed) and np.array_equal(got_key, ek) and np.array_equal(extra, ee) and has.all()
    table.close()


# ---- 5. the doors on tests/golden/text_small.json -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    ids = list(j["corpus"])
    n = len(ids)
    src = ["wiki", "arxiv", "web", "forum"]
    columns = {"src": [None if i % 13 == 4 else src[(i * 7) % 4 if i % 3 else 0] for i in range(n)],
               "year": np.array([1990 + (i * 5) % 40 for i in range(n)], dtype=np.int32),
               "stamp": np.ma.array(((np.arange(n, dtype=np.int64) * 7919) % 1000 - 500) * 2 ** 33, mask=np.arange(n) % 11 == 5),
               "price": np.array([np.nan if i % 19 == 7 else (i * 37) % 101 / 4 for i in range(n)], dtype=np.float32),
               "tags": [[t for b, t in enumerate(("a", "b", "c")) if (i >> b) & 1] for i in range(n)],
               "flag": np.arange(n) % 3 == 0}
    text_of = lambda doc: doc.get("text", doc.get("content", doc.get("body", "")))  # the field the index reads
    toks = {d: set(re.findall(r"\b\w+\b", text_of(j["corpus"][d]).lower())) for d in ids}
    return j, ids, columns, toks


def _value(columns, name, i):
    """What a door returns for row i of a column: None for a doc without a value (a NaN is one)"""
    v = columns[name][i]
    if v is None or v is np.ma.masked or (name == "price" and np.isnan(v)):
        return None
    return v if name == "src" else bool(v) if name == "flag" else float(v) if name == "price" else int(v)


def _expected_sorted(ids, columns, name, docs, order, nulls, top_k):
    """The restatement over doc ids: a sorted() in the header's order over ``docs``, from the Python columns"""
    row = {d: i for i, d in enumerate(ids)}
    vals = {d: _value(columns, name, row[d]) for d in docs}
    sign = 1 if order == "asc" else -1
    if name == "src":
        codes = {s: c for c, s in enumerate(sorted({s for s in columns["src"] if s is not None}))}
        num = {d: None if v is None else codes[v] for d, v in vals.items()}
    else:
        num = vals
    kept = [d for d in docs if num[d] is not None or nulls != "drop"]
    key = lambda d: ((0 if nulls == "first" else 1), 0, row[d]) if num[d] is None else ((1 if nulls == "first" else 0), sign * num[d], row[d])
    return {d: vals[d] for d in sorted(kept, key=key)[:top_k]}


@pytest.mark.parametrize("make", ["service", "bm25", "registry"])
def test_search_sorted_doors(text, make, tmp_path):
    import sparse_rx
    j, ids, columns, toks = text
    queries = {q: j["queries"][q] for q in list(j["queries"])[:6]}
    queries["oov"], queries["blank"] = "zzzunknownzzz", "  "
    if make == "service":
        o = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
        o.build_bm25_index(j["corpus"])
        search = o.search_bm25
    else:
        o = sparse_rx.OptimizedBM25Retriever(device=DEVICE) if make == "bm25" else sparse_rx.OptimizedRetriever({"type": "bm25"}, device=DEVICE, cache_dir=str(tmp_path))
        o.build_index_from_corpus(j["corpus"])
        search = o.search
    with pytest.raises(ValueError, match=r"search_sorted\(\.\.\.\) needs the docs' fields: call set_doc_fields"):
        o.search_sorted(queries, "year")
    o.set_doc_fields(columns)
    q_toks = {q: re.findall(r"\b\w+\b", t.lower()) for q, t in queries.items()}
    any_set = {q: [d for d in ids if set(q_toks[q]) & toks[d]] for q in queries}
    all_set = {q: [d for d in ids if q_toks[q] and all(t in toks[d] for t in q_toks[q])] for q in queries}

    def check(got, doc_sets, name, order="desc", nulls="last", top_k=10):
        assert list(got) == list(doc_sets)
        for q, docs in doc_sets.items():
            want = _expected_sorted(ids, columns, name, docs, order, nulls, top_k)
            assert list(got[q].items()) == list(want.items()), (q, name, order, nulls)
            assert all(type(a) is type(b) for a, b in zip(got[q].values(), want.values()))

    for name in ("year", "stamp", "price", "src", "flag"):
        for order in ("asc", "desc"):
            for nulls in ("last", "first", "drop"):
                check(o.search_sorted(queries, name, order=order, nulls=nulls, top_k=12), any_set, name, order, nulls, 12)  # match="any" is the default
    check(o.search_sorted(queries, "stamp", match="all"), all_set, "stamp")
    check(o.search_sorted(queries, "year", match=None, top_k=400), {q: ids for q in queries}, "year", top_k=400)
    got = o.search_sorted(queries, "src", order="asc", match=None, top_k=len(ids))  # a category orders alphabetically
    strings = [v for v in got["q0"].values() if v is not None]
    assert strings == sorted(strings) and len(set(strings)) == 4 and list(got["q0"].values())[-1] is None
    assert o.search_sorted(queries, "year")["oov"] == {} and o.search_sorted(queries, "year")["blank"] == {}
    # chained with the doc, term and field keywords
    gone = ids[::3]
    word = sorted(set().union(*toks.values()))[5]
    keep = lambda d: d not in set(gone) and word not in toks[d] and columns["year"][ids.index(d)] >= 2000
    got = o.search_sorted(queries, "price", order="asc", excluded_docs=gone, must_not_terms=[word], where=[{"field": "year", "gte": 2000}], top_k=20)
    check(got, {q: [d for d in any_set[q] if keep(d)] for q in queries}, "price", "asc", top_k=20)
    got = o.search_sorted(queries, "stamp", match=None, allowed_docs={"q0": ids[:50]}, where={"q1": [{"field": "src", "eq": "wiki"}]}, top_k=30)
    want = {q: ids for q in queries}
    want["q0"], want["q1"] = ids[:50], [d for i, d in enumerate(ids) if columns["src"][i] == "wiki"]
    check(got, want, "stamp", top_k=30)
    with pytest.raises(ValueError, match="match=\"any\".*any_terms"):
        o.search_sorted(queries, "year", any_terms=[word])
    with pytest.raises(ValueError, match="unknown field 'nope'"):
        o.search_sorted(queries, "nope")
    with pytest.raises(ValueError, match="set column"):
        o.search_sorted(queries, "tags")
    # sort_results of a search against a Python sorted (stable: equal years keep their relevance order)
    res = search(queries, top_k=25)
    row = {d: i for i, d in enumerate(ids)}
    for order, sign in (("asc", 1), ("desc", -1)):
        got = o.sort_results(res, "year", order=order)
        for q in queries:
            want = sorted(res[q], key=lambda d: sign * int(columns["year"][row[d]]))
            assert list(got[q].items()) == [(d, res[q][d]) for d in want], (q, order)
    got = o.sort_results(res, "src", order="asc", nulls="drop", top_k=5)
    for q in queries:
        want = sorted((d for d in res[q] if columns["src"][row[d]] is not None), key=lambda d: columns["src"][row[d]])[:5]
        assert list(got[q].items()) == [(d, res[q][d]) for d in want]
    with pytest.raises(ValueError, match="unknown doc id"):
        o.sort_results({"q0": {"no such doc": 1.0}}, "year")
    o.close()


def test_top_k_above_the_list_depth_pages(text):
    """About 1 300 docs, top_k = 1 200: a page of 1 024, then the cursor"""
    import sparse_rx
    j, ids, columns, toks = text
    corpus = {f"{d}_{r}": j["corpus"][d] for r in range(5) for d in ids}
    big = dict(list(corpus.items())[:1300])
    big_ids = list(big)
    n = len(big_ids)
    cols = {"year": np.array([1990 + (i * 5) % 40 for i in range(n)], dtype=np.int32),
            "stamp": np.ma.array((np.arange(n, dtype=np.int64) * 7919) % 997, mask=np.arange(n) % 11 == 5)}
    o = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    o.build_bm25_index(big)
    o.set_doc_fields(cols)
    q = {"q0": j["queries"]["q0"], "q1": j["queries"]["q1"]}
    for name, nulls in (("year", "last"), ("stamp", "first"), ("stamp", "drop")):
        got = o.search_sorted(q, name, order="desc", nulls=nulls, match=None, top_k=1200)
        want = _expected_sorted(big_ids, cols, name, big_ids, "desc", nulls, 1200)
        assert len(want) == (1200 if nulls != "drop" else min(1200, n - len(range(5, n, 11))))
        for qid in q:
            assert list(got[qid].items()) == list(want.items()), (name, nulls)
    table = o._be.field_table()
    doc, key, has, extra = table.top_by("stamp", 5, order="asc", nulls="first")
    assert extra.tolist() == [[5, 0, n]] and doc.tolist() == [[5, 16, 27, 38, 49]] and not has.any() and key.dtype == np.int64
    doc, key, has, extra = table.top_by("year", 3, order="asc", after=[0])  # doc 0 holds 1990: the next docs that do
    assert key.dtype == np.int32 and has.all() and extra[0, 2] == n and (key == 1990).all() and doc.tolist() == [[8, 16, 24]]
    o.close()
