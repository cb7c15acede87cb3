"""Facet counts without a GPU: the eleventh header and its symbol table, every refusal of both entry points (none reaches a
device), the restatement (tests/facets_ref.py) on a 40-doc table worked by hand, the resolution of binning specs to exact bounds,
the decode and ordering of the doors over a stub table, the Python refusals and the mirrors with the doors not called."""
import ctypes
import inspect
import json
import math
import os
import re
import tempfile
from fractions import Fraction

import numpy as np
import pytest
import torch

import facets_ref
import sparse_rx
from facets_ref import CODES, EDGES, F32, I32, I64, LABELS, SET64
from sparse_rx import _capi, fields
from sparse_rx.backend import SparseBackend, facet_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(16)]  # 16-byte aligned addresses, never dereferenced
I32_MAX, I64_MIN, I64_MAX = 2 ** 31 - 1, -(2 ** 63), 2 ** 63 - 1


def test_eleventh_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_facets.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef SPARSE_RX_FACETS_H")[1]))
    assert declared == set(_capi.FACET_SYMBOLS) == {"srx_facet_counts", "srx_facet_counts_lists"}
    assert '#include "sparse_rx_fields.h"' in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS, _capi.MMR_SYMBOLS,
              _capi.TERMS_SYMBOLS, _capi.MAXSIM_SYMBOLS, _capi.FIELDS_SYMBOLS, _capi.COLLAPSE_SYMBOLS)
    assert [len(t) for t in others] == [35, 4, 4, 8, 5, 3, 2, 3, 1, 1]
    for other in others:
        assert not set(_capi.FACET_SYMBOLS) & set(other)
    assert sum(len(t) for t in others) + len(_capi.FACET_SYMBOLS) == 68
    assert len([f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")]) == 11
    assert "facets.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "sparse_rx_facets.h") in _capi._deps()
    assert "include/sparse_rx_facets.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read().split('"""')[1]
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.FACET_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    for name, value in (("SRX_FACET_CODES", 0), ("SRX_FACET_LABELS", 1), ("SRX_FACET_EDGES", 2)):
        assert re.search(rf"\b{name} = {value}\b", hdr) and getattr(_capi, name) == value == getattr(facets_ref, name.split("_", 2)[2])
    assert re.search(r"#define SRX_FACET_MAX_BINS 8192\b", hdr) and _capi.SRX_FACET_MAX_BINS == 8192 == facets_ref.MAX_BINS
    assert (facets_ref.I32, facets_ref.I64, facets_ref.F32, facets_ref.SET64) == (_capi.SRX_FIELD_I32, _capi.SRX_FIELD_I64, _capi.SRX_FIELD_F32,
                                                                                 _capi.SRX_FIELD_SET64)
    assert ctypes.sizeof(_capi.FacetBins) == 24 and _capi.FacetBins.origin.offset == 8 and _capi.FacetBins.edges.offset == 16


# ---- every refusal of both calls ------------------------------------------------------------------------------------------------
def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, msg, word)


def _col(data, valid, typ):
    return ctypes.pointer(_capi.FieldColDesc(data=data, valid=valid, type=typ))


def _bins(mode, n_bins, origin=0, edges=None):
    return ctypes.pointer(_capi.FacetBins(mode=mode, n_bins=n_bins, origin=origin, edges=edges))


def _flt(bits, n_filters=2, q_filter=None):
    return ctypes.pointer(_capi.DocFilterDesc(bits=bits, n_filters=n_filters, q_filter=q_filter))


def _shared_refusals(call):
    """What both entry points check of the column, n_docs and the bins"""
    _refused(call(col=None), "null col")
    for typ in (-1, 4, 99):
        _refused(call(col=_col(P[0], None, typ)), "unknown column type")
    for typ in (0, 1, 2, 3):
        _refused(call(col=_col(None, None, typ)), "null data")
    for typ, off in ((0, 2), (0, 1), (2, 2), (1, 4), (1, 2), (3, 4)):
        _refused(call(col=_col(P[0] + off, None, typ)), "aligned for its type")
    for off in (4, 8, 2):
        _refused(call(col=_col(P[0], P[1] + off, 0)), "validity row must be 16-byte aligned")
    for n in (0, -3, 2 ** 31 - 1, 2 ** 40):
        _refused(call(n_docs=n), "n_docs must be in [1, 2^31 - 2]")
    _refused(call(bins=None), "null bins")
    for mode in (-1, 3, 99):
        _refused(call(bins=_bins(mode, 4)), "unknown bins mode")
    for typ in (2, 3):
        _refused(call(col=_col(P[0], None, typ), bins=_bins(CODES, 4)), "SRX_FACET_CODES is for I32 and I64 columns")
    for typ in (0, 1, 2):
        _refused(call(col=_col(P[0], None, typ), bins=_bins(LABELS, 4)), "SRX_FACET_LABELS is for SET64 columns")
    _refused(call(col=_col(P[0], None, 3), bins=_bins(EDGES, 4, edges=P[3])), "SRX_FACET_EDGES is for I32, I64 and F32 columns")
    for n in (0, -1, 8193, I32_MAX):
        _refused(call(bins=_bins(CODES, n)), "n_bins must be in [1, 8192]")
        _refused(call(bins=_bins(EDGES, n, edges=P[3])), "n_bins must be in [1, 8192]")
    for n in (0, -1, 65, 8192):
        _refused(call(col=_col(P[0], None, 3), bins=_bins(LABELS, n)), "n_bins must be in [1, 64]")
    _refused(call(bins=_bins(EDGES, 4, edges=None)), "null edges")
    for off in (4, 2, 1):
        _refused(call(bins=_bins(EDGES, 4, edges=P[3] + off)), "edges must be 8-byte aligned")


def test_row_form_refusals():
    L = _capi.lib()
    ok = dict(device=0, col=_col(P[0], P[1], 0), n_docs=1000, bins=_bins(CODES, 8), filter=_flt(P[2], 2, P[4]), n_rows=3, out_counts=P[5],
              out_extra=P[6], stream=None)
    call = lambda **kw: L.srx_facet_counts(*{**ok, **kw}.values())
    _shared_refusals(call)
    _refused(call(n_rows=-1), "n_rows < 0")
    _refused(call(filter=_flt(None)), "null filter bits")
    for off in (4, 8):
        _refused(call(filter=_flt(P[2] + off)), "filter rows must be 16-byte aligned")
    for n in (0, -1):
        _refused(call(filter=_flt(P[2], n)), "n_filters must be >= 1")
    for name in ("out_counts", "out_extra"):
        _refused(call(**{name: None}), "null out_counts / out_extra")
    assert b"srx_facet_counts:" in L.srx_last_error()
    # nothing to do: no launch, whatever the pointers are; the checks still come first
    assert call(n_rows=0) == 0 and call(n_rows=0, filter=None, out_counts=None, out_extra=None) == 0
    assert call(n_rows=0, col=_col(P[0] + 4, None, 2), bins=_bins(EDGES, 8192, edges=P[3] + 8)) == 0  # natural alignment is enough
    assert call(n_rows=0, col=_col(P[0] + 8, None, 3), bins=_bins(LABELS, 64)) == 0
    _refused(call(n_rows=0, bins=_bins(CODES, 0)), "n_bins")
    _refused(call(n_rows=0, filter=_flt(P[2], 0)), "n_filters")


def test_list_form_refusals():
    L = _capi.lib()
    ok = dict(device=0, col=_col(P[0], P[1], 1), n_docs=1000, doc_base=0, bins=_bins(CODES, 8), cand_doc=P[2], cand_count=P[3], nq=3, m=100,
              out_counts=P[5], out_extra=P[6], stream=None)
    call = lambda **kw: L.srx_facet_counts_lists(*{**ok, **kw}.values())
    _shared_refusals(call)
    _refused(call(doc_base=-1), "negative doc_base")
    _refused(call(doc_base=2 ** 31 - 1 - 1000), "doc_base + n_docs must be below 2^31 - 1")
    _refused(call(doc_base=2 ** 40), "doc_base + n_docs must be below 2^31 - 1")
    _refused(call(nq=-1), "nq < 0")
    for m in (0, -1):
        _refused(call(m=m), "m must be >= 1")
    _refused(call(nq=2 ** 16, m=2 ** 15), "nq * m")
    _refused(call(cand_doc=None), "null cand_doc")
    for name in ("out_counts", "out_extra"):
        _refused(call(**{name: None}), "null out_counts / out_extra")
    assert b"srx_facet_counts_lists:" in L.srx_last_error()
    assert call(nq=0) == 0 and call(nq=0, cand_doc=None, cand_count=None, out_counts=None, out_extra=None) == 0
    assert call(nq=0, doc_base=2 ** 31 - 2 - 1000, m=I32_MAX) == 0
    _refused(call(nq=0, m=0), "m must be >= 1")


# ---- the restatement on a table worked by hand -----------------------------------------------------------------------------------
def _hand():
    """40 docs.  year (I32) = 2000 + d % 10, so every year four times; the docs 0 (2000) and 39 (2009) have no value.
    big (I64) = (d % 4 - 2) * 2^40: -2^41, -2^40, 0, 2^40 ten times each.  x (F32) = d / 2, but doc 7 holds a NaN and doc 8 a -0.0.
    tags (SET64) = d % 8, three labels; doc 1 has no value."""
    d = np.arange(40)
    year, year_ok = (2000 + d % 10).astype(np.int32), np.ones(40, bool)
    year_ok[[0, 39]] = False
    big = ((d % 4 - 2) * 2 ** 40).astype(np.int64)
    x = (d / 2).astype(np.float32)
    x[7], x[8] = np.nan, -0.0
    tags, tags_ok = (d % 8).astype(np.int64), np.ones(40, bool)
    tags_ok[1] = False
    return year, year_ok, big, x, tags, tags_ok


def _f32_edges(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32).astype(np.int64)


def test_restatement_by_hand():
    year, year_ok, big, x, tags, tags_ok = _hand()
    first20 = np.arange(40) < 20
    masks = np.stack([first20, np.ones(40, bool)])
    # CODES on year, origin 2003, bins 2003 .. 2006; row 0 = the docs 0 .. 19 (every year twice), row 1 = every doc, row 2 = no filter
    c, e = facets_ref.facet_counts(I32, year, year_ok, CODES, 4, 2003, None, masks, [0, 1, -1], 3)
    assert c.tolist() == [[2, 2, 2, 2], [4, 4, 4, 4], [4, 4, 4, 4]] and e.tolist() == [[1, 11, 20], [2, 22, 40], [2, 22, 40]]
    # q_filter None: every output row is row 0
    c, e = facets_ref.facet_counts(I32, year, year_ok, CODES, 4, 2003, None, masks, None, 2)
    assert c.tolist() == [[2, 2, 2, 2]] * 2 and e.tolist() == [[1, 11, 20]] * 2
    # EDGES on year: [2000, 2002) holds 3 + 4 docs, [2002, 2002) none, [2002, 2008) 24, [2008, 2009) 4; 2009 is the last edge: other
    c, e = facets_ref.facet_counts(I32, year, year_ok, EDGES, 4, 0, [2000, 2002, 2002, 2008, 2009])
    assert c.tolist() == [[7, 0, 24, 4]] and e.tolist() == [[2, 3, 40]]
    # without the validity row the two docs carry their stored years
    c, e = facets_ref.facet_counts(I32, year, None, EDGES, 4, 0, [2000, 2002, 2002, 2008, 2009])
    assert c.tolist() == [[8, 0, 24, 4]] and e.tolist() == [[0, 4, 40]]
    # I64: values and origins that differ only above bit 32
    c, e = facets_ref.facet_counts(I64, big, None, CODES, 3, -(2 ** 41))
    assert c.tolist() == [[10, 0, 0]] and e.tolist() == [[0, 30, 40]]
    c, e = facets_ref.facet_counts(I64, big, None, EDGES, 2, 0, [-(2 ** 41), 0, 2 ** 40 + 1])
    assert c.tolist() == [[20, 20]] and e.tolist() == [[0, 0, 40]]
    c, e = facets_ref.facet_counts(I64, big, None, CODES, 8192, I64_MIN)
    assert c.sum() == 0 and e.tolist() == [[0, 40, 40]]
    assert facets_ref.bin_codes(I64_MAX, I64_MIN, 8192) == -1 and facets_ref.bin_codes(I64_MIN + 5, I64_MIN, 8192) == 5  # nothing wraps
    # F32: the NaN is in no bin, -0.0 is in [0, 5)
    c, e = facets_ref.facet_counts(F32, x, None, EDGES, 3, 0, _f32_edges([0.0, 5.0, 10.0, 20.0]))
    assert c.tolist() == [[9, 10, 20]] and e.tolist() == [[0, 1, 40]]
    c, e = facets_ref.facet_counts(F32, x, None, EDGES, 2, 0, _f32_edges([0.5, 0.5, 19.5]), masks, [0], 1)
    assert c.tolist() == [[0, 17]] and e.tolist() == [[0, 3, 20]]  # the docs 0 and 8 lie below, the NaN nowhere
    # LABELS: bit 0 in 20 docs, one of them without a value; no bit in the 5 docs with d % 8 == 0
    c, e = facets_ref.facet_counts(SET64, tags, tags_ok, LABELS, 3)
    assert c.tolist() == [[19, 20, 20]] and e.tolist() == [[1, 5, 40]]
    c, e = facets_ref.facet_counts(SET64, tags, tags_ok, LABELS, 2)
    assert c.tolist() == [[19, 20]] and e.tolist() == [[1, 10, 40]]
    for mode, cc, ee in ((LABELS, c, e),):
        facets_ref.check_invariants(mode, cc, ee)
    # lists: 40 and -1 lie outside, doc 0 twice counts twice (both times without a value)
    lists = np.array([[0, 0, 5, 39, 40, -1, 13]], dtype=np.int32)
    c, e = facets_ref.facet_counts_lists(I32, year, year_ok, CODES, 4, 0, lists, None, 2003)
    assert c.tolist() == [[1, 0, 1, 0]] and e.tolist() == [[3, 0, 5]]
    for count, counts, extra in ((3, [0, 0, 1, 0], [2, 0, 3]), (0, [0] * 4, [0] * 3), (-2, [0] * 4, [0] * 3), (99, [1, 0, 1, 0], [3, 0, 5])):
        c, e = facets_ref.facet_counts_lists(I32, year, year_ok, CODES, 4, 0, lists, [count], 2003)
        assert c.tolist() == [counts] and e.tolist() == [extra]
    c, e = facets_ref.facet_counts_lists(I32, year, year_ok, CODES, 4, 100, np.array([[100, 105, 99, 140, 5]]), None, 2003)
    assert c.tolist() == [[0, 0, 1, 0]] and e.tolist() == [[1, 0, 2]]
    c, e = facets_ref.facet_counts_lists(SET64, tags, tags_ok, LABELS, 3, 0, np.array([[7, 7, 1, 8, 3]]), None)
    assert c.tolist() == [[3, 3, 2]] and e.tolist() == [[1, 1, 5]]
    facets_ref.check_invariants(LABELS, c, e)


def test_both_invariants_on_random_tables():
    for seed in range(30):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(1, 200))
        valid = rng.random(n) > 0.2
        masks = rng.random((3, n)) < 0.5
        i32 = rng.integers(-5, 20, n).astype(np.int32)
        for mode, kw in ((CODES, dict(origin=int(rng.integers(-6, 6)))), (EDGES, dict(edges=sorted(int(v) for v in rng.integers(-8, 25, 8))))):
            c, e = facets_ref.facet_counts(I32, i32, valid, mode, 7, filter_masks=masks, q_filter=[0, 1, 2, -1], n_rows=4, **kw)
            facets_ref.check_invariants(mode, c, e)
            assert (e[:, 2] == [masks[0].sum(), masks[1].sum(), masks[2].sum(), n]).all()
        sets = rng.integers(0, 2 ** 10, n).astype(np.int64)
        c, e = facets_ref.facet_counts(SET64, sets, valid, LABELS, 6, filter_masks=masks, q_filter=[2], n_rows=1)
        facets_ref.check_invariants(LABELS, c, e)
        sel = masks[2] & valid
        assert c.sum() == sum(bin(int(v) & 63).count("1") for v in sets[sel]) and e[0, 1] == sum(1 for v in sets[sel] if not int(v) & 63)


# ---- binning specs resolved to exact bounds --------------------------------------------------------------------------------------
def _schema():
    n = 8
    return fields.host_columns({"year": np.arange(n, dtype=np.int32), "big": np.arange(n, dtype=np.int64), "flag": np.arange(n) % 2 == 0,
                                "src": ["a", "b", None, "a", "b", "a", "b", "c"], "price": np.ones(n, np.float32),
                                "tags": [["x"], ["y", "z"]] * 4})


def test_default_specs():
    s = _schema()
    f = fields.check_facet_args(s, "src")
    assert (f.mode, f.n_bins, f.origin, f.edges, f.values) == (CODES, 3, 0, None, ["a", "b", "c"])
    f = fields.check_facet_args(s, "flag")
    assert (f.mode, f.n_bins, f.origin, f.values) == (CODES, 2, 0, [False, True])
    f = fields.check_facet_args(s, "tags")
    assert (f.mode, f.n_bins, f.values) == (LABELS, 3, ["x", "y", "z"])  # a set column's label count
    f = fields.check_facet_args(s, "year", {"origin": -3, "bins": 5})
    assert (f.mode, f.n_bins, f.origin, f.values) == (CODES, 5, -3, [-3, -2, -1, 0, 1])
    f = fields.check_facet_args(s, "big", {"origin": I64_MIN, "bins": 8192})
    assert (f.n_bins, f.origin) == (8192, I64_MIN)
    for name in ("src", "flag", "tags"):
        with pytest.raises(ValueError, match="takes no spec"):
            fields.check_facet_args(s, name, {"edges": [0, 1]})
    for name, spec in (("year", None), ("big", {}), ("price", None), ("price", {"origin": 0, "bins": 4}), ("year", {"origin": 0}),
                       ("year", {"edges": [0, 1], "bins": 3})):
        with pytest.raises(ValueError, match="give"):
            fields.check_facet_args(s, name, spec)
    with pytest.raises(ValueError, match="unknown field 'nope'"):
        fields.check_facet_args(s, "nope")
    for bad in (0, -1, 8193):
        with pytest.raises(ValueError, match="bins"):
            fields.check_facet_args(s, "year", {"origin": 0, "bins": bad})
    for bad in (dict(origin=1.5, bins=3), dict(origin=0, bins=True), dict(origin=2 ** 63, bins=3)):
        with pytest.raises(ValueError, match="origin|bins"):
            fields.check_facet_args(s, "big", bad)
    many = fields.HostColumn("category", np.zeros(4, np.int32), None, [f"v{i:05d}" for i in range(8193)])
    with pytest.raises(ValueError, match="8193 distinct values"):
        fields.check_facet_args({"c": many}, "c")
    assert fields.check_facet_args({"c": fields.HostColumn("category", np.zeros(4, np.int32), None, [f"v{i:05d}" for i in range(8192)])}, "c").n_bins == 8192


def test_float_edges_resolve_to_the_float32_at_or_above():
    s = _schema()
    given = [0.1, 1 / 3, 0.7, 1, 2.5, 16777217, 1e39]
    f = fields.check_facet_args(s, "price", {"edges": given})
    assert f.mode == EDGES and f.n_bins == 6 and f.edges.dtype == np.int64 and f.values == list(zip(given, given[1:]))
    got = facets_ref.edges_as_f32(f.edges)
    assert (f.edges >> 32 == 0).all()
    for e, r in zip(given, got):
        below = np.nextafter(r, np.float32(-np.inf))
        if math.isinf(r):
            assert e > 3.4028235e38
        else:
            assert Fraction(float(r)) >= Fraction(e) and Fraction(float(below)) < Fraction(e), (e, r)
    assert float(got[2]) > 0.7 and float(got[0]) > 0.1 and got[5] == np.float32(16777218) and got[3] == 1 and got[4] == np.float32(2.5)
    # so bin [0.7, 1) holds exactly the float32 values >= 0.7: np.float32(0.7) itself lies below 0.7
    assert facets_ref.bin_edges_f32(np.float32(0.7), got, 6) == 1 and facets_ref.bin_edges_f32(got[2], got, 6) == 2
    f = fields.check_facet_args(s, "price", {"edges": [-math.inf, -1e39, -0.0, 0.0, math.inf]})
    got = facets_ref.edges_as_f32(f.edges)
    assert got[0] == -np.inf and got[1] == np.float32(-3.4028235e38) and got[4] == np.inf and f.n_bins == 4


def test_int_edges_resolve_to_the_integer_at_or_above():
    s = _schema()
    f = fields.check_facet_args(s, "year", {"edges": [-0.5, 0.5, 2, 2.0, 2.5, 7.000001]})
    assert f.edges.tolist() == [0, 1, 2, 2, 3, 8] and f.values[0] == (-0.5, 0.5) and f.n_bins == 5
    # beyond the int32 limits: an int64 entry stands for the edge as it is; beyond int64 below: every value lies above it
    f = fields.check_facet_args(s, "year", {"edges": [-(2 ** 70), -(2 ** 40), 2 ** 31, 2 ** 40, 2 ** 70, math.inf]})
    assert f.edges.tolist() == [I64_MIN, -(2 ** 40), 2 ** 31, 2 ** 40, I64_MAX, I64_MAX]
    f = fields.check_facet_args(s, "big", {"edges": [-math.inf, -(2 ** 63) - 1, -(2 ** 63), I64_MAX - 0, I64_MAX]})
    assert f.edges.tolist() == [I64_MIN, I64_MIN, I64_MIN, I64_MAX, I64_MAX]
    for bad in (2 ** 63, 2.0 ** 63, math.inf, 1e30):  # no int64 entry stands for "above every int64"
        with pytest.raises(ValueError, match="above the int64 range"):
            fields.check_facet_args(s, "big", {"edges": [0, bad]})


def test_edges_refusals():
    s = _schema()
    for name in ("year", "big", "price"):
        for bad in ([1, 0], [0, 1, 0.5], [0, math.nan], [math.nan, 1], [0], [], "01", 5, [0, "1"], [0, None]):
            with pytest.raises(ValueError, match="edges|edge"):
                fields.check_facet_args(s, name, {"edges": bad})
        with pytest.raises(ValueError, match="8193 bins"):
            fields.check_facet_args(s, name, {"edges": list(range(8194))})
        assert fields.check_facet_args(s, name, {"edges": list(range(8193))}).n_bins == 8192
        assert fields.check_facet_args(s, name, {"edges": [3, 3]}).n_bins == 1  # equal neighbours are legal: an empty bin


# ---- the doors over a stub table ---------------------------------------------------------------------------------------------------
def test_facet_dict_decode_and_order():
    s = _schema()
    fs = fields.check_facet_args(s, "src")
    assert facet_dict(fs, np.array([2, 5, 2]), (1, 0, 10)) == {"counts": {"b": 5, "a": 2, "c": 2}, "missing": 1, "other": 0, "total": 10}
    assert list(facet_dict(fs, np.array([2, 5, 2]), (1, 0, 10))["counts"]) == ["b", "a", "c"]  # by count, then by bin
    assert facet_dict(fs, np.array([2, 5, 2]), (1, 0, 10), top=2)["counts"] == {"b": 5, "a": 2}
    assert facet_dict(fs, np.array([0, 0, 4]), (0, 0, 4), top=1)["counts"] == {"c": 4}  # empty bins are not listed
    assert facet_dict(fs, None, (0, 0, 0), top=3) == {"counts": {}, "missing": 0, "other": 0, "total": 0}
    fe = fields.check_facet_args(s, "price", {"edges": [0, 0.5, 2]})
    assert facet_dict(fe, np.array([1, 3]), (0, 2, 6))["counts"] == {(0.5, 2): 3, (0, 0.5): 1}
    fy = fields.check_facet_args(s, "year", {"origin": 2000, "bins": 3})
    got = facet_dict(fy, np.array([4, 0, 4], dtype=np.int32), np.array([0, 1, 9], dtype=np.int32))
    assert got == {"counts": {2000: 4, 2002: 4}, "missing": 0, "other": 1, "total": 9} and all(type(v) is int for v in got["counts"].values())


class _StubTable:
    """facet_device / facet_lists_device answered by the restatement on CPU tensors; it records its calls"""

    def __init__(self, cols):
        self.cols, self.device, self.calls = cols, torch.device("cpu"), []

    def facet_device(self, column, spec, filter=None, q_filter=None, n_rows=None):
        self.calls.append((column, filter, q_filter, n_rows))
        c = self.cols[column]
        out = facets_ref.facet_counts(c.type, c.data, c.valid, spec.mode, spec.n_bins, spec.origin, spec.edges, None, None, n_rows)
        return tuple(torch.from_numpy(x) for x in out)

    def facet_lists_device(self, column, doc, count, spec):
        self.calls.append((column, tuple(doc.shape)))
        c = self.cols[column]
        out = facets_ref.facet_counts_lists(c.type, c.data, c.valid, spec.mode, spec.n_bins, 0, doc.numpy(), count.numpy(), spec.origin, spec.edges)
        return tuple(torch.from_numpy(x) for x in out)


def _stub_backend():
    be = SparseBackend("cuda:0", 14)
    be._fields = _schema()
    table = _StubTable(be._fields)
    be.field_table = lambda: table
    be.host = type("Host", (), {"doc_ids": [f"d{i}" for i in range(8)], "vocabulary": {}, "n_docs": 8})()
    be.dev = object()
    return be, table


def test_backend_doors_over_a_stub_table():
    be, table = _stub_backend()
    queries = {"q0": "anything", "q1": ""}
    got = be.facets(queries, {"src": None, "year": {"edges": [0, 2.5, 8]}, "tags": None}, match=None)
    want = {"src": {"counts": {"a": 3, "b": 3, "c": 1}, "missing": 1, "other": 0, "total": 8},
            "year": {"counts": {(2.5, 8): 5, (0, 2.5): 3}, "missing": 0, "other": 0, "total": 8},
            "tags": {"counts": {"x": 4, "y": 4, "z": 4}, "missing": 0, "other": 0, "total": 8}}
    assert got == {"q0": want, "q1": want} and list(got["q0"]["year"]["counts"]) == [(2.5, 8), (0, 2.5)]
    assert table.calls == [("src", None, None, 1), ("year", None, None, 1), ("tags", None, None, 1)]  # one launch per field, one row for all
    assert be.facets(queries, "src", match=None, top=1)["q1"]["src"]["counts"] == {"a": 3}
    assert be.facets(queries, ["flag"], match=None)["q0"]["flag"]["counts"] == {False: 4, True: 4}
    # a text without a token has the empty set under "any" / "all", and nothing is launched for it
    table.calls.clear()
    got = be.facets({"q1": " "}, ["src"])
    assert got == {"q1": {"src": {"counts": {}, "missing": 0, "other": 0, "total": 0}}} and table.calls == []
    # the list form: d2 has no src, d7 is the one "c"; a doc listed twice counts twice
    got = be.facets_of({"q0": {"d0": 3.0, "d2": 2.0, "d7": 1.0}, "q1": {}, "v": [{"doc_id": "d7", "score": 1.0}, {"doc_id": "d7", "score": 0.5}]}, ["src"], top=1)
    assert got["q0"]["src"] == {"counts": {"a": 1}, "missing": 1, "other": 0, "total": 3}
    assert got["q1"]["src"]["total"] == 0 and got["v"]["src"] == {"counts": {"c": 2}, "missing": 0, "other": 0, "total": 2}
    assert be.facets_of({}, ["src"]) == {}
    with pytest.raises(ValueError, match="unknown doc id 'zz'"):
        be.facets_of({"q0": {"zz": 1.0}}, ["src"])


def test_backend_refusals():
    be, table = _stub_backend()
    q = {"q0": "w"}
    with pytest.raises(ValueError, match=r"match=\"any\" puts the query's own terms into the any list; give match=None \(or \"all\"\) with any_terms="):
        be.facets(q, ["src"], any_terms=["w"])
    with pytest.raises(ValueError, match=r"match=\"any\""):
        be.facets(q, ["src"], match="any", any_terms={"q0": ["w"]})
    with pytest.raises(ValueError, match="match must be"):
        be.facets(q, ["src"], match="some")
    with pytest.raises(ValueError, match="unknown field 'nope'"):
        be.facets(q, ["src", "nope"])
    with pytest.raises(ValueError, match="at least one field"):
        be.facets(q, [])
    with pytest.raises(ValueError, match="takes no spec"):
        be.facets(q, {"src": {"edges": [0, 1]}})
    for door, arg in ((be.facets, q), (be.facets_of, {"q0": {"d0": 1.0}})):
        with pytest.raises(ValueError, match="top must be >= 1"):
            door(arg, ["src"], top=0)
    with pytest.raises(ValueError, match="must_terms must be a sequence"):
        be.facets(q, ["src"], match="all", must_terms="w")
    assert table.calls == []
    be._fields = None
    for door, arg in ((be.facets, q), (be.facets_of, {"q0": {"d0": 1.0}})):
        with pytest.raises(ValueError, match=r"facets(_of)?\(\.\.\.\) needs the docs' fields: call set_doc_fields"):
            door(arg, ["src"])


def test_field_table_refusals():
    cols = _schema()
    t = fields.FieldTable(cols, {name: (torch.from_numpy(c.data), None) for name, c in cols.items()}, torch.device("cpu"))
    doc = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="unknown field 'nope'"):
        t.facet_device("nope")
    with pytest.raises(ValueError, match="unknown field 'nope'"):
        t.facet_lists_device("nope", doc, None)
    with pytest.raises(ValueError, match="give"):
        t.facet_device("year")
    with pytest.raises(ValueError, match="q_filter picks rows of a filter"):
        t.facet_device("src", q_filter=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="q_filter picks rows of a filter"):
        t.facet("src", q_filter=[0, 1])
    with pytest.raises(ValueError, match="filter must be a DocFilter"):
        t.facet_device("src", filter=object())
    with pytest.raises(ValueError, match=r"int32 tensor \[nq, m >= 1\]"):
        t.facet_lists_device("src", doc.long(), None)
    with pytest.raises(ValueError, match=r"int32 tensor \[nq, m >= 1\]"):
        t.facet_lists_device("src", torch.zeros((2, 0), dtype=torch.int32), None)
    with pytest.raises(ValueError, match=r"count must be an int32 tensor \[nq\]"):
        t.facet_lists_device("src", doc, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="doc is on meta"):
        t.facet_lists_device("src", doc.to("meta"), None)
    with pytest.raises(ValueError, match="2-D integer array"):
        t.facet_lists("src", np.zeros(4, np.int32))
    t.close()
    with pytest.raises(ValueError, match="the table is closed"):
        t.facet_device("src")


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def one_rank_group():
    import torch.distributed as dist
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method=f"file://{os.path.join(tmp, 'rendezvous')}", rank=0, world_size=1)
        try:
            yield
        finally:
            dist.destroy_process_group()


def test_mirrors_untouched_when_the_doors_are_not_called(golden_dir, one_rank_group, tmp_path):
    """The fake backend of test_dict_search_cpu.py (the CPU oracle behind the sharding protocol, counting its searches): searches
    run and cache as before, with and without fields; the facet doors refuse without fields and on a sharded index, before any
    search or launch."""
    from test_dict_search_cpu import _Counted
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    q = {qid: j["queries"][qid] for qid in ("q0", "q1", "q2")}
    n = len(j["corpus"])
    for make, method in ((lambda f: sparse_rx.RetrievalService(shard_searcher_factory=f, sharded=True), "search_bm25"),
                         (lambda f: sparse_rx.OptimizedBM25Retriever(shard_searcher_factory=f, sharded=True), "search"),
                         (lambda f: sparse_rx.OptimizedRetriever({"type": "bm25"}, shard_searcher_factory=f, sharded=True, cache_dir=str(tmp_path)), "search")):
        f = _Counted()
        o = make(f)
        with pytest.raises(ValueError, match="not built"):
            o.facets(q, ["src"])
        with pytest.raises(ValueError, match="not built"):
            o.facets_of({}, ["src"])
        (o.build_bm25_index if method == "search_bm25" else o.build_index_from_corpus)(j["corpus"])
        search = getattr(o, method)
        r = search(q, top_k=10)
        assert f.take() == [(3, 10)] and len(o.query_cache) == 3 and all(r[qid] for qid in q)
        for door, arg in ((o.facets, q), (o.facets_of, r)):
            with pytest.raises(ValueError, match=r"facets(_of)?\(\.\.\.\) needs the docs' fields: call set_doc_fields"):
                door(arg, ["src"])
        o.set_doc_fields({"src": ["s%d" % (i % 3) for i in range(n)], "price": np.ones(n, np.float32)})
        for door, arg in ((o.facets, q), (o.facets_of, r)):
            with pytest.raises(ValueError, match="needs the whole index on one GPU"):
                door(arg, ["src"])
        assert search(q, top_k=10) == r and f.take() == [] and len(o.query_cache) == 3
        o.close()


def test_doors_and_their_defaults():
    for cls in (sparse_rx.RetrievalService, sparse_rx.OptimizedBM25Retriever, sparse_rx.OptimizedRetriever):
        sig = inspect.signature(cls.facets).parameters
        assert list(sig)[:3] == ["self", "queries", "fields"]
        want = dict(match="any", allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None, must_not_terms=None, operators=False, where=None,
                    top=None)
        assert {k: sig[k].default for k in want} == want and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
        assert list(inspect.signature(cls.facets_of).parameters)[:3] == ["self", "results", "fields"]
        assert "superset" in cls.facets.__doc__ and "score > 0" in cls.facets.__doc__
    for cls in (sparse_rx.HybridRetriever, sparse_rx.ShardedSearcher, sparse_rx.HostBatchPipeline):
        assert not hasattr(cls, "facets") and not hasattr(cls, "facets_of")
    for name in ("facet_device", "facet_lists_device", "facet", "facet_lists"):
        assert callable(getattr(fields.FieldTable, name))
