"""Facet counts on the GPU (include/sparse_rx_facets.h).  Expected counts are never the engine's own: the restatement
(tests/facets_ref.py) over the column, the masks and the lists a call was given.  Every comparison is exact, both invariants
are asserted on every case, and every output buffer is pre-filled with 0x7F7F7F7F so that a word the call does not write shows.

The kernel's sizes (csrc/facets.hip): in a call with 2 048 or more (row, 2 048-doc chunk) pairs a wave's unit is 8 192 docs, a
workgroup's chunk 32 768 and a segment at least 16 docs per bin (four chunks = 131 072 docs at 8 192 bins).  A smaller call
flushes after 2 docs per bin and halves the unit -- 4 096, 2 048, 1 024, 512 docs; chunks of 16 384 .. 2 048 -- while a chunk is
longer than that segment (a call with 2 048 pairs or more always keeps the 8 192-doc unit): with one row, 8 192 / 4 096 / 2 048 / up to 1 024 bins give chunks of 16 384 / 8 192 / 4 096 / 2 048 docs.
Histograms of up to 1 024 bins take the small instance (edges in LDS), larger ones the 8 192-bin one."""
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

import facets_ref  # noqa: E402
from facets_ref import CODES, EDGES, F32, I32, I64, LABELS, SET64  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -(2 ** 31), 2 ** 31 - 1, -(2 ** 63), 2 ** 63 - 1
GARBAGE = 0x7F7F7F7F
UNIT, CHUNK = 8192, 32768   # of a call that fills the chip
MIN_UNIT = 512               # the smallest unit: every unit size is a multiple of it
MANY = 2100                  # rows that make any table a call with >= 2 048 (row, chunk) pairs
DTYPE = {I32: np.int32, I64: np.int64, F32: np.float32, SET64: np.int64}


def _f32_edges(values):
    """float32 edges as the int64 entries of the header: the float's bits in the low 32"""
    return np.asarray(values, dtype=np.float32).view(np.uint32).astype(np.int64)


class _Col:
    """One column on the device, as the C calls take it, next to its host arrays"""

    def __init__(self, col_type, data, valid=None, doc_base=0):
        import torch
        from sparse_rx import _capi
        from sparse_rx.filter import pack_masks
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.type, self.data = col_type, np.ascontiguousarray(data, dtype=DTYPE[col_type])
        self.valid = None if valid is None else np.asarray(valid, dtype=bool)
        self.n_docs, self.doc_base = len(self.data), doc_base
        self.data_t = torch.from_numpy(self.data).to(DEVICE)
        self.valid_t = None if valid is None else torch.from_numpy(pack_masks(self.valid).view(np.int32).copy()).to(DEVICE).reshape(-1)
        self.desc = _capi.FieldColDesc(data=self.data_t.data_ptr(), valid=None if valid is None else self.valid_t.data_ptr(), type=col_type)
        self._bins = {}

    def bins(self, mode, n_bins, origin, edges):
        key = (mode, n_bins, origin, None if edges is None else np.asarray(edges).tobytes())
        if key not in self._bins:
            self._bins[key] = facets_ref.doc_bins(self.type, self.data, mode, n_bins, origin, edges)
        return self._bins[key]

    def _bins_struct(self, mode, n_bins, origin, edges):
        import torch
        from sparse_rx import _capi
        e_t = None if edges is None else torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int64)).to(DEVICE)
        return _capi.FacetBins(mode=mode, n_bins=n_bins, origin=origin, edges=None if e_t is None else e_t.data_ptr()), e_t

    def rows(self, mode, n_bins, origin=0, edges=None, masks=None, q_filter=None, n_rows=1, bits=None, stream=None, outs=None, label=""):
        """srx_facet_counts on garbage-filled outputs against the restatement.  masks: bool[n_filters, n_docs] or None (a NULL
        filter); bits: the packed rows to upload in place of pack_masks(masks) (to set bits the contract says are not read)."""
        import ctypes
        import torch
        from sparse_rx import _capi
        from sparse_rx.filter import pack_masks
        b, e_t = self._bins_struct(mode, n_bins, origin, edges)
        fdesc = keep = None
        if masks is not None:
            packed = pack_masks(np.asarray(masks, dtype=bool)) if bits is None else bits
            bits_t = torch.from_numpy(packed.view(np.int32).copy()).to(DEVICE)
            q_t = None if q_filter is None else torch.from_numpy(np.ascontiguousarray(q_filter, dtype=np.int32)).to(DEVICE)
            keep = _capi.DocFilterDesc(bits=bits_t.data_ptr(), n_filters=int(bits_t.shape[0]), q_filter=None if q_t is None else q_t.data_ptr())
            fdesc = ctypes.byref(keep)
        if outs is None:
            outs = (torch.full((n_rows, n_bins), GARBAGE, dtype=torch.int32, device=DEVICE), torch.full((n_rows, 3), GARBAGE, dtype=torch.int32, device=DEVICE))
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        rc = _capi.lib().srx_facet_counts(0, ctypes.byref(self.desc), self.n_docs, ctypes.byref(b), fdesc, n_rows, outs[0].data_ptr(), outs[1].data_ptr(), sp)
        _capi.check(rc, "srx_facet_counts")
        torch.cuda.synchronize()
        counts, extra = outs[0].cpu().numpy(), outs[1].cpu().numpy()
        # the restatement, once per distinct base row
        ref_bins = self.bins(mode, n_bins, origin, edges)
        picks = [0 if q_filter is None else int(q) for q in (range(n_rows) if q_filter is None else q_filter)] if masks is not None else [-1] * n_rows
        memo = {}
        for r, pick in enumerate(picks):
            if pick not in memo:
                memo[pick] = facets_ref.facet_counts(self.type, self.data, self.valid, mode, n_bins, origin, edges,
                                                     None if pick < 0 else np.asarray(masks)[pick: pick + 1], None, 1, bins=ref_bins)
            ec, ee = memo[pick]
            assert np.array_equal(counts[r], ec[0]), (label, "counts", r, pick, np.flatnonzero(counts[r] != ec[0])[:8])
            assert np.array_equal(extra[r], ee[0]), (label, "extra", r, pick, extra[r], ee[0])
        facets_ref.check_invariants(mode, counts, extra)
        return counts, extra, outs

    def lists(self, mode, n_bins, doc, count, origin=0, edges=None, stream=None, label=""):
        import ctypes
        import torch
        from sparse_rx import _capi
        b, e_t = self._bins_struct(mode, n_bins, origin, edges)
        doc = np.ascontiguousarray(doc, dtype=np.int32)
        nq, m = doc.shape
        d_t = torch.from_numpy(doc).to(DEVICE)
        c_t = None if count is None else torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).to(DEVICE)
        outs = (torch.full((nq, n_bins), GARBAGE, dtype=torch.int32, device=DEVICE), torch.full((nq, 3), GARBAGE, dtype=torch.int32, device=DEVICE))
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        rc = _capi.lib().srx_facet_counts_lists(0, ctypes.byref(self.desc), self.n_docs, self.doc_base, ctypes.byref(b), d_t.data_ptr(),
                                                None if c_t is None else c_t.data_ptr(), nq, m, outs[0].data_ptr(), outs[1].data_ptr(), sp)
        _capi.check(rc, "srx_facet_counts_lists")
        torch.cuda.synchronize()
        counts, extra = outs[0].cpu().numpy(), outs[1].cpu().numpy()
        ec, ee = facets_ref.facet_counts_lists(self.type, self.data, self.valid, mode, n_bins, self.doc_base, doc, count, origin, edges,
                                               bins=self.bins(mode, n_bins, origin, edges))
        assert np.array_equal(counts, ec), (label, "counts", np.argwhere(counts != ec)[:8])
        assert np.array_equal(extra, ee), (label, "extra", extra[:4], ee[:4])
        facets_ref.check_invariants(mode, counts, extra)
        return counts, extra


def _masks(rng, n_docs, densities=(0.5, 1.0, 1e-3, 0.0)):
    m = np.zeros((len(densities), n_docs), dtype=bool)
    for i, p in enumerate(densities):
        m[i] = rng.random(n_docs) < p
    if n_docs > 1:
        m[0, 0], m[0, -1] = True, True
    return m


def _holes(n_docs, rng=None, p=0.1):
    """A validity row that misses the first and the last doc of the table and of every unit and chunk, whatever the unit size"""
    valid = np.ones(n_docs, dtype=bool) if rng is None else rng.random(n_docs) > p
    d = np.arange(n_docs)
    valid[(d % MIN_UNIT == 0) | (d % MIN_UNIT == MIN_UNIT - 1) | (d == n_docs - 1)] = False
    return valid


# ---- 1. geometries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 63, 64, 65, 129, 2047, 2048, 2049, UNIT - 1, UNIT, UNIT + 1, 20011, CHUNK - 1, CHUNK, CHUNK + 1])
def test_geometry(n_docs):
    rng = np.random.default_rng(n_docs)
    col = _Col(I32, rng.integers(-1, 6, n_docs), _holes(n_docs, rng) if n_docs > 2 else None)
    masks = _masks(rng, n_docs)
    col.rows(CODES, 5, masks=masks, q_filter=[0, 1, 2, 3, -1, 1, 0], n_rows=7, label=f"n_docs={n_docs}")                # 512-doc units
    col.rows(CODES, 5, masks=masks, q_filter=rng.integers(-1, 4, MANY), n_rows=MANY, label=f"n_docs={n_docs}, 8192-doc units")
    col.rows(CODES, 5, label="null filter")
    col.rows(CODES, 5, masks=masks[:1], label="row 0")


@pytest.mark.parametrize("n_docs", [4 * CHUNK - 1, 4 * CHUNK, 4 * CHUNK + 1])
def test_segment_borders_and_every_doc_in_its_own_bin(n_docs):
    """8 192 bins and 40 rows (65 chunks of 2 048 docs x 40 >= 2 048: 8 192-doc units, 16 docs per bin): a segment is four chunks, so
    these tables are one segment minus a doc, one segment, and a second segment of one doc; 16 docs per bin at most, and under the
    sparse row every counted doc is alone in its bin.  With 3 rows the same tables are a small call: 16 384-doc chunks, one per segment."""
    rng = np.random.default_rng(n_docs)
    col = _Col(I32, np.arange(n_docs) % 8192 + 100, _holes(n_docs))
    masks = _masks(rng, n_docs, (0.5, 1e-3))
    masks[1, -1] = True
    col.rows(CODES, 8192, origin=100, masks=masks, q_filter=rng.integers(-1, 2, 40), n_rows=40, label=f"n_docs={n_docs}, 40 rows")
    col.rows(CODES, 8192, origin=100, masks=masks, q_filter=[0, 1, -1], n_rows=3, label=f"n_docs={n_docs}, 3 rows")


@pytest.mark.parametrize("n_bins,chunk", [(64, 2048), (1024, 2048), (2048, 4096), (4096, 8192), (8192, 16384)])
def test_small_calls_at_every_unit_size(n_bins, chunk):
    """One and three rows: the unit shrinks until a chunk is no longer than 2 docs per bin; tables of one chunk - 1 / exact / + 1 and
    of five chunks + 1"""
    rng = np.random.default_rng(n_bins)
    for n_docs in (chunk - 1, chunk, chunk + 1, 5 * chunk + 1):
        col = _Col(I32, rng.integers(-2, n_bins + 2, n_docs), _holes(n_docs, rng))
        masks = _masks(rng, n_docs, (0.5, 1e-3, 1.0))
        col.rows(CODES, n_bins, masks=masks[:1], label=f"one row, n_docs={n_docs}")
        col.rows(CODES, n_bins, masks=masks, q_filter=[1, 2, -1], n_rows=3, label=f"three rows, n_docs={n_docs}")


def test_segments_grow_with_the_rows():
    """5 chunks x 1 000 rows: the launch rule makes a segment two chunks (5 * 1000 / 2048), so the table is walked as 2 + 2 + 1"""
    n_docs = 4 * CHUNK + 7
    rng = np.random.default_rng(3)
    col = _Col(I32, rng.integers(0, 9, n_docs))
    masks = _masks(rng, n_docs, (0.5, 1e-3, 0.0))
    col.rows(CODES, 9, masks=masks, q_filter=rng.integers(-1, 3, 1000), n_rows=1000)


# ---- 2. types and modes -------------------------------------------------------------------------------------------------------
def _type_cases(n_docs, rng):
    i32 = rng.integers(-50, 50, n_docs)
    i64 = rng.integers(-50, 50, n_docs).astype(np.int64) * (2 ** 33 + 1)
    f32 = (rng.standard_normal(n_docs) * 10).astype(np.float32)
    sets = rng.integers(0, 2 ** 63, n_docs, dtype=np.int64) & rng.integers(0, 2 ** 63, n_docs, dtype=np.int64)
    int_edges = np.array([-60, -20, -20, 0, 7, 49, 50], dtype=np.int64)
    return [(I32, i32, CODES, 64, -40, None), (I32, i32, EDGES, 6, 0, int_edges),
            (I64, i64, CODES, 100, -3 * (2 ** 33 + 1), None), (I64, i64, EDGES, 6, 0, int_edges * (2 ** 33 + 1)),
            (F32, f32, EDGES, 5, 0, _f32_edges([-np.inf, -3.5, 0.0, 0.25, 12.0, np.inf])),
            (SET64, sets, LABELS, 64, 0, None), (SET64, sets, LABELS, 17, 0, None)]


@pytest.mark.parametrize("case", range(7))
def test_every_type_with_every_legal_mode(case):
    n_docs = 2 * CHUNK + UNIT + 77
    rng = np.random.default_rng(100 + case)
    col_type, data, mode, n_bins, origin, edges = _type_cases(n_docs, rng)[case]
    masks = _masks(rng, n_docs, (0.5, 1e-3, 1.0))
    for valid in (None, _holes(n_docs, rng)):
        col = _Col(col_type, data, valid)
        col.rows(mode, n_bins, origin, edges, masks=masks, q_filter=[0, 1, 2, -1], n_rows=4, label=f"case {case}")
        lists = rng.integers(-3, n_docs + 3, (5, 300))
        col.lists(mode, n_bins, lists, [300, 0, 150, -1, 999], origin, edges, label=f"case {case} lists")


# ---- 3. bin counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8192])
def test_bin_counts(n_bins):
    n_docs = 20011
    rng = np.random.default_rng(n_bins)
    masks = _masks(rng, n_docs, (1.0, 0.5))
    own = _Col(I32, np.arange(n_docs) % (n_bins + 1) + 5)  # every bin, and one value past the last
    own.rows(CODES, n_bins, origin=5, masks=masks, q_filter=[0, 1], n_rows=2, label="spread")
    one = _Col(I32, np.full(n_docs, n_bins + 4))           # every doc in ONE bin: the last one
    counts, extra, _ = one.rows(CODES, n_bins, origin=5, masks=masks, q_filter=[0, 1], n_rows=2, label="one bin")
    assert counts[0, n_bins - 1] == n_docs and extra[0].tolist() == [0, 0, n_docs]
    skew = _Col(I64, np.where(rng.random(n_docs) < 0.9, 3, rng.integers(0, n_bins, n_docs)))
    skew.rows(CODES, n_bins, masks=masks, q_filter=[0, 1, -1], n_rows=3, label="skew")
    # edges: bin j = [3 j, 3 j + 3)
    e = _Col(I32, rng.integers(-5, 3 * n_bins + 5, n_docs))
    e.rows(EDGES, n_bins, edges=np.arange(n_bins + 1, dtype=np.int64) * 3, masks=masks, q_filter=[0, 1], n_rows=2, label="edges")
    f = _Col(F32, rng.integers(-5, 3 * n_bins + 5, n_docs).astype(np.float32) + np.float32(0.5))
    f.rows(EDGES, n_bins, edges=_f32_edges(np.arange(n_bins + 1) * 3), masks=masks[1:], label="f32 edges")
    e.lists(EDGES, n_bins, rng.integers(0, n_docs, (3, 500)), None, edges=np.arange(n_bins + 1, dtype=np.int64) * 3, label="edges lists")


# ---- 4. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 2, 17, 257])
def test_row_counts_and_q_filter(n_rows):
    n_docs = 20011
    rng = np.random.default_rng(n_rows)
    col = _Col(I32, rng.integers(0, 40, n_docs), _holes(n_docs, rng))
    masks = _masks(rng, n_docs, (0.0, 1.0, 0.5, 1e-3, 0.5))
    col.rows(CODES, 33, masks=masks, q_filter=rng.integers(-1, 5, n_rows), n_rows=n_rows, label="picked")
    if n_rows <= 5:
        col.rows(CODES, 33, masks=masks, q_filter=np.arange(n_rows), n_rows=n_rows, label="in order")
    col.rows(CODES, 33, n_rows=n_rows, label="null filter: every row is every doc")
    col.rows(CODES, 33, masks=masks[2:3], n_rows=n_rows, label="null q_filter: every row is row 0")


def test_more_rows_than_the_grid_has():
    n_docs, n_rows = 33, 65535 + 4
    rng = np.random.default_rng(9)
    col = _Col(I32, rng.integers(0, 3, n_docs), rng.random(n_docs) > 0.2)
    col.rows(CODES, 2, masks=_masks(rng, n_docs, (0.5, 1.0, 0.1)), q_filter=rng.integers(-1, 3, n_rows), n_rows=n_rows)


@pytest.mark.parametrize("n_docs", [1, 33, 100, 2049, 20011])
def test_bits_at_or_above_n_docs_are_never_counted(n_docs):
    from sparse_rx.filter import pack_masks
    rng = np.random.default_rng(n_docs)
    col = _Col(I32, rng.integers(0, 4, n_docs))
    masks = _masks(rng, n_docs, (0.5, 0.0))
    bits = pack_masks(masks).copy()
    tail = ~pack_masks(np.ones((2, n_docs), dtype=bool))  # the tail of the last word and the padding words
    bits |= tail
    assert (bits[:, -1] != 0).all() or n_docs % 128 == 0
    col.rows(CODES, 4, masks=masks, q_filter=[0, 1], n_rows=2, bits=bits)


# ---- 5. values ----------------------------------------------------------------------------------------------------------------
def test_int64_values_and_origins():
    hi = 2 ** 32
    data = np.array([5, 5 + hi, 5 + 2 * hi, 5 - hi, 6 + hi, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, 0, -1, 7 + hi], dtype=np.int64)
    col = _Col(I64, data, np.array([True] * 11 + [False]))
    for origin in (5, 5 + hi, 5 - hi, 4 + hi, I64_MIN, I64_MAX, I64_MAX - 1, I64_MIN + 1, 0, -1):
        for n_bins in (1, 2, 3, 8192):
            col.rows(CODES, n_bins, origin=origin, label=f"origin={origin} n_bins={n_bins}")
            col.lists(CODES, n_bins, np.arange(-1, 13)[None], None, origin=origin)
    # origin = INT64_MIN with a value at INT64_MAX: no bin, nothing wraps
    counts, extra, _ = col.rows(CODES, 8192, origin=I64_MIN)
    assert counts[0, 0] == 1 and counts[0, 1] == 1 and counts.sum() == 2 and extra[0].tolist() == [1, 9, 12]
    e = np.array([I64_MIN, 5 - hi, 5, 5, 5 + hi, I64_MAX], dtype=np.int64)
    col.rows(EDGES, 5, edges=e)
    col.rows(EDGES, 1, edges=np.array([I64_MIN, I64_MAX], dtype=np.int64))
    col.rows(EDGES, 1, edges=np.array([I64_MAX, I64_MAX], dtype=np.int64))


def test_int32_limits():
    data = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX], dtype=np.int32)
    col = _Col(I32, data)
    for origin in (I32_MIN, I32_MAX, I32_MAX - 1, I32_MIN - 1, I32_MAX + 1, I64_MIN, I64_MAX, -1):
        col.rows(CODES, 3, origin=origin, label=f"origin={origin}")
    col.rows(EDGES, 4, edges=np.array([I32_MIN, I32_MIN + 1, 0, I32_MAX, I32_MAX + 1], dtype=np.int64))
    col.rows(EDGES, 2, edges=np.array([I64_MIN, 0, I64_MAX], dtype=np.int64))


def test_float_specials_against_edges_at_those_values():
    tiny = np.float32(1e-45)  # the smallest denormal
    vals = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, tiny, -tiny, np.float32(1.1754942e-38), 1.0, -1.0, 3.4028235e38, -3.4028235e38, 0.5],
                    dtype=np.float32)
    col = _Col(F32, vals, np.array([True] * 13 + [False]))
    for edges in ([-np.inf, -tiny, -0.0, tiny, np.inf], [-np.inf, np.inf], [np.inf, np.inf], [-np.inf, -np.inf], [0.0, 0.0, 0.0], [-0.0, 0.0, tiny, tiny, 1.0],
                  [-3.4028235e38, -1.0, 1.0, 3.4028235e38], [1.0, 1.0], [-1.0, 1.0]):
        counts, extra, _ = col.rows(EDGES, len(edges) - 1, edges=_f32_edges(edges), label=str(edges))
        col.lists(EDGES, len(edges) - 1, np.arange(14)[None].repeat(2, 0), [14, 7], edges=_f32_edges(edges))
    # [-inf, inf): everything but the NaNs and +inf; a NaN has a value and lands in no bin
    counts, extra, _ = col.rows(EDGES, 1, edges=_f32_edges([-np.inf, np.inf]))
    assert counts[0, 0] == 10 and extra[0].tolist() == [1, 3, 14]


def test_set_values():
    data = np.array([0, 1, 2 ** 63 - 1, -1, I64_MIN, I64_MIN + 1, 2 ** 62, 5, 0, -1], dtype=np.int64)  # I64_MIN = bit 63 alone, -1 = all ones
    col = _Col(SET64, data, np.array([True] * 8 + [False, False]))
    for n_bins in (1, 2, 63, 64):
        counts, extra, _ = col.rows(LABELS, n_bins, label=f"n_bins={n_bins}")
        col.lists(LABELS, n_bins, np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3, 3]]), None)
    counts, extra, _ = col.rows(LABELS, 64)
    assert counts[0, 63] == 3 and counts[0, 0] == 5 and extra[0].tolist() == [2, 1, 10]
    counts, extra, _ = col.rows(LABELS, 63)
    assert extra[0].tolist() == [2, 2, 10]  # bit 63 alone is no counted label


# ---- 6. lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1024, 3000])
def test_lists(m):
    n_docs, base = 6001, 1000
    rng = np.random.default_rng(m)
    col = _Col(I32, rng.integers(0, 70, n_docs), rng.random(n_docs) > 0.1, doc_base=base)
    nq = 9
    doc = rng.integers(base, base + n_docs, (nq, m)).astype(np.int64)
    outside = np.array([-1, base - 1, base + n_docs, base + n_docs + 7, 0, I32_MAX, I32_MIN], dtype=np.int64)
    hit = rng.random((nq, m)) < 0.1
    doc[hit] = rng.choice(outside, size=int(hit.sum()))
    doc[1, :] = doc[1, 0]        # one doc m times
    doc[2, m // 2:] = doc[2, 0]  # a doc twice and more
    count = np.array([m, 0, m, -1, m + 5, I32_MAX, I32_MIN, m // 2, 1], dtype=np.int32)
    count[1] = m
    for n_bins in (64, 3, 1025):
        col.lists(CODES, n_bins, doc, count, label=f"m={m} n_bins={n_bins}")
        col.lists(CODES, n_bins, doc, None, label=f"m={m} n_bins={n_bins} null count")
    col.lists(CODES, 64, doc[:1], np.array([0], dtype=np.int32), label="an empty list")


# ---- 7. execution -------------------------------------------------------------------------------------------------------------
def test_side_stream_and_second_call():
    import torch
    n_docs = 3 * CHUNK + 5
    rng = np.random.default_rng(77)
    col = _Col(I32, rng.integers(0, 300, n_docs), _holes(n_docs, rng))
    masks = _masks(rng, n_docs)
    side = torch.cuda.Stream(device=DEVICE)
    c1, e1, outs = col.rows(CODES, 300, masks=masks, q_filter=[0, 1, 2, 3], n_rows=4, stream=side)
    c2, e2, _ = col.rows(CODES, 300, masks=masks, q_filter=[0, 1, 2, 3], n_rows=4, outs=outs)  # into the buffers that hold a result
    assert np.array_equal(c1, c2) and np.array_equal(e1, e2)
    col.rows(CODES, 300, masks=masks, q_filter=[3, 2, 1, 0], n_rows=4, outs=outs)                # and another result over them
    col.lists(CODES, 300, rng.integers(0, n_docs, (4, 700)), None, stream=side)


# ---- 8. cross-checks with the row builders and the search ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    ids = list(j["corpus"])
    n = len(ids)
    src = ["wiki", "arxiv", "web", "forum"]
    columns = {"src": [None if i % 13 == 4 else src[(i * 7) % 4 if i % 3 else 0] for i in range(n)],
               "year": np.array([1990 + (i * 5) % 40 for i in range(n)], dtype=np.int32),
               "price": np.array([(i * 37) % 101 / 4 for i in range(n)], dtype=np.float32),
               "tags": [None if i % 17 == 3 else [t for b, t in enumerate(("a", "b", "c")) if (i >> b) & 1] for i in range(n)],
               "flag": np.arange(n) % 3 == 0}
    text_of = lambda doc: doc.get("text", doc.get("content", doc.get("body", "")))  # the field the index reads
    toks = {d: set(re.findall(r"\b\w+\b", text_of(j["corpus"][d]).lower())) for d in ids}
    return j, ids, columns, toks


def _expected_facet(ids, columns, name, docs, spec=None, top=None):
    """The dict a door returns for the doc ids ``docs`` (a list: a doc named twice counts twice), from the Python columns"""
    col = columns[name]
    counts, missing, other = {}, 0, 0
    order = {}
    if name == "src":
        order = {v: i for i, v in enumerate(sorted({s for s in col if s is not None}))}
    elif name == "tags":
        order = {v: i for i, v in enumerate(("a", "b", "c"))}
    elif name == "flag":
        order = {False: 0, True: 1}
    elif "edges" in spec:
        order = {(a, b): i for i, (a, b) in enumerate(zip(spec["edges"], spec["edges"][1:]))}
    else:
        order = {spec["origin"] + i: i for i in range(spec["bins"])}
    row = {d: i for i, d in enumerate(ids)}
    for d in docs:
        v = col[row[d]]
        if v is None:
            missing += 1
        elif name == "tags":
            if not v:
                other += 1
            for t in v:
                counts[t] = counts.get(t, 0) + 1
        else:
            if name == "flag":
                key = bool(v)
            elif name == "src":
                key = v
            elif "edges" in spec:
                key = next(((a, b) for a, b in order if a <= float(v) < b), None)
            else:
                key = int(v) if int(v) in order else None
            if key is None:
                other += 1
            else:
                counts[key] = counts.get(key, 0) + 1
    listed = sorted(counts, key=lambda k: (-counts[k], order[k]))
    return {"counts": {k: counts[k] for k in (listed if top is None else listed[:top])}, "missing": missing, "other": other, "total": len(docs)}


FIELDS = {"src": None, "year": {"origin": 1995, "bins": 30}, "price": {"edges": [0, 2.5, 2.5, 10, 25.25]}, "tags": None, "flag": None}
YEAR_EDGES = {"year": {"edges": [1990, 2000.5, 2010, 2029]}}


def test_field_table_doors_against_the_builders(text):
    import torch
    import sparse_rx
    from sparse_rx import fields
    j, ids, columns, toks = text
    n = len(ids)
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    table = fields.FieldTable.from_columns(columns, device=DEVICE)
    host = fields.host_columns(columns)
    # rows of FieldTable.filter and of term_filter, counted; total == DocFilter.count()
    where = [{"must": [{"field": "year", "gte": 2000}]}, {"must_not": [{"field": "src", "eq": "wiki"}]}, {"should": [{"field": "tags", "any_of": ["a", "c"]}]}]
    f_rows = table.filter(where)
    year = columns["year"]
    f_masks = np.array([year >= 2000, [s != "wiki" for s in columns["src"]], [t is not None and bool({"a", "c"} & set(t)) for t in columns["tags"]]])
    words = sorted(svc.vocabulary)[:3]
    t_rows = svc.dev.term_filter([[svc.vocabulary[words[0]]], []], [[], [svc.vocabulary[w] for w in words]], [[], []])
    t_masks = np.array([[words[0] in toks[d] for d in ids], [bool(set(words) & toks[d]) for d in ids]])
    for flt, masks in ((f_rows, f_masks), (t_rows, t_masks)):
        for name, spec in {**FIELDS, **{"year2": None}}.items():
            if name == "year2":
                name, spec = "year", YEAR_EDGES["year"]
            fs = fields.check_facet_args(host, name, spec)
            counts, extra = table.facet(name, spec, filter=flt)
            c = host[name]
            ec, ee = facets_ref.facet_counts(c.type, c.data, c.valid, fs.mode, fs.n_bins, fs.origin, fs.edges, masks, np.arange(len(masks)), len(masks))
            assert np.array_equal(counts, ec) and np.array_equal(extra, ee), name
            assert np.array_equal(extra[:, 2], flt.count()) and np.array_equal(extra[:, 2], masks.sum(axis=1))
            facets_ref.check_invariants(fs.mode, counts, extra)
        counts, extra = table.facet("src", filter=flt, q_filter=[1, -1, 0, 1])
        assert extra[:, 2].tolist() == [int(masks[1].sum()), n, int(masks[0].sum()), int(masks[1].sum())]
    counts, extra = table.facet("flag")
    assert counts.tolist() == [[n - len(range(0, n, 3)), len(range(0, n, 3))]] and extra.tolist() == [[0, 0, n]]
    counts, extra = table.facet("flag", n_rows=3)
    assert counts.shape == (3, 2) and (extra[:, 2] == n).all()
    # the list form over a search result
    from sparse_rx.index import _batch_to_device, encode_queries
    d, s, c = svc.dev.search_device(*_batch_to_device(torch, *encode_queries(list(j["queries"].values()), svc.vocabulary), DEVICE), 50)
    for name, spec in FIELDS.items():
        fs = fields.check_facet_args(host, name, spec)
        counts, extra = (t.cpu().numpy() for t in table.facet_lists_device(name, d, c, spec))
        col = host[name]
        ec, ee = facets_ref.facet_counts_lists(col.type, col.data, col.valid, fs.mode, fs.n_bins, 0, d.cpu().numpy(), c.cpu().numpy(), fs.origin, fs.edges)
        assert np.array_equal(counts, ec) and np.array_equal(extra, ee) and np.array_equal(extra[:, 2], c.cpu().numpy()), name
        h_counts, h_extra = table.facet_lists(name, d.cpu().numpy(), c.cpu().numpy(), spec)
        assert np.array_equal(h_counts, ec) and np.array_equal(h_extra, ee)
    with pytest.raises(ValueError, match="unknown field 'nope'"):
        table.facet("nope")
    svc.close()


# ---- 9. the doors on tests/golden/text_small.json -------------------------------------------------------------------------------
@pytest.mark.parametrize("make", ["service", "bm25", "registry"])
def test_facets_doors(text, make, tmp_path):
    import sparse_rx
    j, ids, columns, toks = text
    queries = {q: j["queries"][q] for q in list(j["queries"])[:8]}
    queries["oov"], queries["blank"] = "zzzunknownzzz", "  "
    if make == "service":
        o = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
        o.build_bm25_index(j["corpus"])
        search = o.search_bm25
    else:
        o = sparse_rx.OptimizedBM25Retriever(device=DEVICE) if make == "bm25" else sparse_rx.OptimizedRetriever({"type": "bm25"}, device=DEVICE, cache_dir=str(tmp_path))
        o.build_index_from_corpus(j["corpus"])
        search = o.search
    with pytest.raises(ValueError, match=r"facets\(\.\.\.\) needs the docs' fields: call set_doc_fields"):
        o.facets(queries, ["src"])
    o.set_doc_fields(columns)
    vocab = set().union(*toks.values())
    q_toks = {q: re.findall(r"\b\w+\b", t.lower()) for q, t in queries.items()}
    any_set = {q: [d for d in ids if set(q_toks[q]) & toks[d]] for q in queries}
    all_set = {q: [d for d in ids if q_toks[q] and all(t in toks[d] for t in q_toks[q])] for q in queries}

    def check(got, doc_sets, fields_spec=FIELDS, top=None):
        assert list(got) == list(doc_sets)
        for q, docs in doc_sets.items():
            assert list(got[q]) == list(fields_spec)
            for name, spec in fields_spec.items():
                want = _expected_facet(ids, columns, name, docs, spec, top)
                assert got[q][name] == want and list(got[q][name]["counts"].items()) == list(want["counts"].items()), (q, name)

    check(o.facets(queries, FIELDS), any_set)                      # match="any" is the default
    check(o.facets(queries, FIELDS, match="all"), all_set)
    check(o.facets(queries, FIELDS, match=None), {q: ids for q in queries})
    check(o.facets(queries, YEAR_EDGES), any_set, YEAR_EDGES)
    check(o.facets(queries, ["src", "flag"], top=2), any_set, {"src": None, "flag": None}, top=2)
    check(o.facets(queries, "tags", top=1), any_set, {"tags": None}, top=1)
    assert any(v["src"]["missing"] for v in o.facets(queries, ["src"]).values()) and o.facets(queries, ["src"])["oov"]["src"]["total"] == 0
    # chained with the doc, term and field keywords
    gone = ids[::3]
    word = sorted(vocab)[5]
    keep = lambda q, d: d not in set(gone) and word not in toks[d] and columns["year"][ids.index(d)] >= 2000
    got = o.facets(queries, FIELDS, excluded_docs=gone, must_not_terms=[word], where=[{"field": "year", "gte": 2000}])
    check(got, {q: [d for d in any_set[q] if keep(q, d)] for q in queries})
    got = o.facets(queries, FIELDS, match=None, allowed_docs={"q0": ids[:50]}, where={"q1": [{"field": "src", "eq": "wiki"}]})
    want = {q: ids for q in queries}
    want["q0"], want["q1"] = ids[:50], [d for i, d in enumerate(ids) if columns["src"][i] == "wiki"]
    check(got, want)
    got = o.facets(queries, ["src"], match=None, any_terms=[word])
    check(got, {q: [d for d in ids if word in toks[d]] for q in queries}, {"src": None})
    with pytest.raises(ValueError, match="match=\"any\".*any_terms"):
        o.facets(queries, ["src"], any_terms=[word])
    with pytest.raises(ValueError, match="unknown field 'nope'"):
        o.facets(queries, ["nope"])
    # every doc of the complete ranking lies in the match="any" set; facets_of over results
    full = search(queries, top_k=len(ids))
    for q in queries:
        assert set(full[q]) <= set(any_set[q])
    res = search(queries, top_k=25)
    check(o.facets_of(res, FIELDS), {q: list(res[q]) for q in queries})
    check(o.facets_of(res, ["src"], top=1), {q: list(res[q]) for q in queries}, {"src": None}, top=1)
    assert o.facets_of({}, ["src"]) == {}
    with pytest.raises(ValueError, match="unknown doc id"):
        o.facets_of({"q0": {"no such doc": 1.0}}, ["src"])
    if make == "service":
        rng = np.random.default_rng(5)
        o.set_embeddings(rng.standard_normal((len(ids), 32)).astype(np.float32))
        live = {q: t for q, t in queries.items() if q not in ("oov", "blank")}
        hyb = o.search_hybrid(live, {q: rng.standard_normal(32).astype(np.float32) for q in live}, top_k=30)
        check(o.facets_of(hyb, FIELDS), {q: list(hyb[q]) for q in live})
        vec = {"v": o.search_by_vector(rng.standard_normal(32).astype(np.float32), k=40, min_score=-100.0)}
        check(o.facets_of(vec, ["src", "tags"]), {"v": [r["doc_id"] for r in vec["v"]]}, {"src": None, "tags": None})
    o.close()
