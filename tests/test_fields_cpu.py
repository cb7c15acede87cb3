"""Field predicates without a GPU: the ninth header and its symbol table, every refusal of the entry point (none reaches a
device), the NumPy restatement (tests/fields_ref.py) on an example worked by hand, the host's clause resolution against exact
arithmetic, columns_from_metadata, the keyword resolution of the API mirrors (field_filter_spec, the combination with doc and term
filters) and the mirrors with no keyword given."""
import ctypes
import json
import math
import os
import re
import tempfile

import numpy as np
import pytest

import fields_ref
import filter_ref
import sparse_rx
from sparse_rx import _capi, fields
from sparse_rx.backend import FieldFilterSpec, doc_filter_spec, field_filter_spec, term_filter_spec
from sparse_rx.fields import WhereResolver, host_column, host_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(16)]  # 16-byte aligned addresses, never dereferenced
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -(2 ** 31), 2 ** 31 - 1, -(2 ** 63), 2 ** 63 - 1


def test_ninth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_fields.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.FIELDS_SYMBOLS) and len(declared) == 1, declared ^ set(_capi.FIELDS_SYMBOLS)
    assert '#include "sparse_rx_filter.h"' in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS, _capi.MMR_SYMBOLS,
              _capi.TERMS_SYMBOLS, _capi.MAXSIM_SYMBOLS)
    assert [len(t) for t in others] == [35, 4, 4, 8, 5, 3, 2, 3]
    for other in others:
        assert not set(_capi.FIELDS_SYMBOLS) & set(other)
    assert sum(len(t) for t in others) + len(_capi.FIELDS_SYMBOLS) == 65
    assert "fields.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "sparse_rx_fields.h") in _capi._deps()
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.FIELDS_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    # the enums and the two structs as the header spells them
    for name, value in (("SRX_FIELD_I32", 0), ("SRX_FIELD_I64", 1), ("SRX_FIELD_F32", 2), ("SRX_FIELD_SET64", 3), ("SRX_FOP_RANGE", 0),
                        ("SRX_FOP_IN", 1), ("SRX_FOP_MASK_ANY", 2), ("SRX_FOP_MASK_ALL", 3)):
        assert re.search(rf"\b{name} = {value}\b", hdr) and getattr(_capi, name) == value
        assert getattr(fields_ref, name.split("_", 2)[2]) == value
    assert ctypes.sizeof(_capi.FieldColDesc) == 24 and _capi.FieldColDesc.valid.offset == 8 and _capi.FieldColDesc.type.offset == 16
    assert sparse_rx.FieldTable is fields.FieldTable and sparse_rx.columns_from_metadata is fields.columns_from_metadata
    assert "FieldTable" in sparse_rx.__all__ and "columns_from_metadata" in sparse_rx.__all__


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, msg)


def _cols(*specs):
    arr = (_capi.FieldColDesc * max(len(specs), 1))()
    for i, (data, valid, typ) in enumerate(specs):
        arr[i].data, arr[i].valid, arr[i].type = data, valid, typ
    return arr


def _base(**kw):
    d = dict(bits=P[8], n_filters=1, q_filter=None)
    d.update(kw)
    return ctypes.byref(_capi.DocFilterDesc(**d))


def test_builder_refusals():
    L = _capi.lib()
    good = _cols((P[0], None, 0), (P[1], P[2], 1), (P[3], None, 2), (P[4], None, 3))
    ok = dict(device=0, n_docs=1000, cols=good, n_cols=4, clauses=P[5], n_clauses=3, values=None, n_rows=3, all_ptr=P[6], all_clause=P[7],
              any_ptr=None, any_clause=None, none_ptr=P[9], none_clause=P[10], base=None, out=P[11], stream=None)
    call = lambda **kw: L.srx_filter_from_fields(*{**ok, **kw}.values())
    for n in (0, -3, 2 ** 31 - 1, 2 ** 40):
        _refused(call(n_docs=n), "n_docs must be in [1, 2^31 - 2]")
    for n in (0, -1, 33):
        _refused(call(n_cols=n), "n_cols must be in [1, 32]")
    _refused(call(cols=None), "null cols")
    _refused(call(cols=_cols((None, None, 0)), n_cols=1), "null data")
    for typ, off in ((0, 2), (2, 1), (1, 4), (3, 4), (1, 2)):
        _refused(call(cols=_cols((P[0] + off, None, typ)), n_cols=1), "aligned for its type")
    assert call(cols=_cols((P[0] + 4, None, 0), (P[1] + 4, None, 2), (P[1] + 8, None, 1)), n_cols=3, n_rows=0) == 0  # natural alignment is enough
    for typ in (-1, 4, 99):
        _refused(call(cols=_cols((P[0], None, typ)), n_cols=1), "unknown column type")
    for off in (4, 8, 2):
        _refused(call(cols=_cols((P[0], P[2] + off, 0)), n_cols=1), "validity row must be 16-byte aligned")
    _refused(call(n_clauses=-1), "n_clauses < 0")
    _refused(call(clauses=None), "null clauses")
    assert call(clauses=None, n_clauses=0, n_rows=0) == 0
    _refused(call(n_rows=-1), "n_rows < 0")
    for half in ("all_ptr", "all_clause", "none_ptr", "none_clause"):
        _refused(call(**{half: None}), "go together")
    _refused(call(any_ptr=P[5]), "go together")
    _refused(call(any_clause=P[5]), "go together")
    _refused(call(out=None), "null out_bits")
    for off in (4, 8, 2):
        _refused(call(out=P[11] + off), "16-byte aligned")
    # the base, by the filter header's rules
    _refused(call(base=_base(bits=None)), "null filter bits")
    _refused(call(base=_base(bits=P[8] + 4)), "16-byte aligned")
    for nf in (0, -1):
        _refused(call(base=_base(n_filters=nf)), "n_filters")
    assert b"srx_filter_from_fields" in L.srx_last_error()
    # nothing to do: no launch, with or without lists and base
    assert call(n_rows=0) == 0
    assert call(n_rows=0, base=_base(), all_ptr=None, all_clause=None, none_ptr=None, none_clause=None) == 0
    _refused(call(n_rows=0, out=None), "null out_bits")  # the checks come first
    # the size of out_bits is the term builder's call: no twin
    assert L.srx_filter_from_terms_bytes(3, 1000) == 3 * 32 * 4


# ---- the restatement on an example worked by hand -------------------------------------------------------------------------------
def _hand():
    """40 docs.  year (I32) = 1990 + d, docs 5 and 6 without a value; views (I64) = (d - 20) * 2^33; price (F32) = d / 4, doc 7 NaN, doc 8
    -0.0, docs 0 and 39 without a value; tags (SET64): bit 0 in the even docs, bit 1 in the multiples of 3, bit 63 in docs >= 31."""
    n = 40
    d = np.arange(n)
    year = (1990 + d).astype(np.int32)
    year_ok = ~np.isin(d, (5, 6))
    views = ((d - 20).astype(np.int64)) << 33
    price = (d / 4).astype(np.float32)
    price[7], price[8] = np.nan, -0.0
    price_ok = ~np.isin(d, (0, 39))
    tags = ((d % 2 == 0).astype(np.uint64) | ((d % 3 == 0).astype(np.uint64) << np.uint64(1)) | ((d >= 31).astype(np.uint64) << np.uint64(63))).view(np.int64)
    cols = [(fields_ref.I32, year, year_ok), (fields_ref.I64, views, None), (fields_ref.F32, price, price_ok), (fields_ref.SET64, tags, None)]
    return n, d, cols


def test_restatement_by_hand():
    n, d, cols = _hand()
    R, IN, ANY, ALL = fields_ref.RANGE, fields_ref.IN, fields_ref.MASK_ANY, fields_ref.MASK_ALL
    fb = fields_ref.bits_of_f32
    values = [2 << 33, -(3 << 33), 2 << 33, 7, fb(0.0), fb(2.5), fb(np.nan)]
    clauses = [(0, R, 2000, 2010),              # 0: year in [2000, 2010]: docs 10..20
               (1, R, -(2 << 33), (2 << 33)),   # 1: views: docs 18..22 -- bounds that differ from 0 only above bit 32
               (1, IN, 0, 4),                   # 2: views in {2^34, -3 * 2^33, 2^34, 7}: docs 22 and 17
               (2, R, fb(0.0), fb(2.0)),        # 3: price in [0, 2]: docs 1..8 but the NaN (7); doc 8 is -0; doc 0 has no value
               (2, IN, 4, 3),                   # 4: price in {0, 2.5, NaN}: doc 8 (-0 == 0) and doc 10
               (3, ANY, 1 | (1 << 63) - (1 << 64), 0),   # 5: even, or >= 31
               (3, ALL, 3, 0),                  # 6: even and a multiple of 3
               (0, R, 2010, 2000),              # 7: lo > hi
               (0, ANY, 1, 0),                  # 8: an op that does not fit the column
               (7, R, 0, 0),                    # 9: a col outside the table
               (1, IN, 0, 0),                   # 10: an empty IN
               (0, R, I64_MIN, I64_MAX)]        # 11: year exists
    hold = lambda c: fields_ref.clause_holds(cols, clauses[c], values, n)
    assert np.flatnonzero(hold(0)).tolist() == list(range(10, 21))
    assert np.flatnonzero(hold(1)).tolist() == [18, 19, 20, 21, 22]
    assert np.flatnonzero(hold(2)).tolist() == [17, 22]
    assert np.flatnonzero(hold(3)).tolist() == [1, 2, 3, 4, 5, 6, 8]
    assert np.flatnonzero(hold(4)).tolist() == [8, 10]
    assert np.array_equal(hold(5), (d % 2 == 0) | (d >= 31)) and np.array_equal(hold(6), d % 6 == 0)
    assert not any(hold(c).any() for c in (7, 8, 9, 10))
    assert np.flatnonzero(~hold(11)).tolist() == [5, 6]
    all_ = [[0], [0, 6], [], [], [], [-1], [], [3], [0], [11, 11]]
    any_ = [[], [], [2, 4], [], [], [], [-1], [-1, 2], [], [7, 1]]
    none = [[], [], [], [11], [], [], [], [-1], [0], [5, 99]]
    m = fields_ref.field_masks(cols, clauses, values, n, all_, any_, none)
    assert m.shape == (10, n)
    assert np.flatnonzero(m[0]).tolist() == list(range(10, 21)) and np.flatnonzero(m[1]).tolist() == [12, 18]
    assert np.flatnonzero(m[2]).tolist() == [8, 10, 17, 22]
    assert np.flatnonzero(m[3]).tolist() == [5, 6]   # a doc without a value passes the clause under none
    assert m[4].all()                                # the empty triple: every doc
    assert not m[5].any() and not m[6].any()         # -1 in all; -1 alone in any: the list is not empty
    assert np.flatnonzero(m[7]).tolist() == []       # price in [0, 2] and views in {..}: none in common; -1 in none has no effect
    assert not m[8].any()                            # a clause in all and in none
    assert np.flatnonzero(m[9]).tolist() == [19, 21]  # year exists, views in range, odd and below 31; id 99 = a clause no doc satisfies
    assert filter_ref.pack(m[1]).tolist() == [(1 << 12) | (1 << 18), 0, 0, 0]
    base = np.stack([d < 20, d >= 20])
    q_base = [0, 1, -1, 0, 1, 0, 0, 1, 0, -1]
    b = fields_ref.field_masks(cols, clauses, values, n, all_, any_, none, base, q_base)
    assert np.flatnonzero(b[0]).tolist() == list(range(10, 20)) and np.flatnonzero(b[1]).tolist() == [] and np.array_equal(b[2], m[2])
    assert np.array_equal(b[4], base[1]) and np.array_equal(b[9], m[9])
    b0 = fields_ref.field_masks(cols, clauses, values, n, all_, None, None, base)
    assert np.array_equal(b0[0], m[0] & base[0]) and np.array_equal(b0[2], base[0])
    # the records of the resolver round-trip through the restatement's tuple form
    rec = np.asarray([[c | (op << 32), lo, hi] for c, op, lo, hi in clauses], dtype=np.int64)
    assert fields_ref.records(rec) == [tuple(int(x) for x in c) for c in clauses]


# ---- the host's clause resolution -----------------------------------------------------------------------------------------------
def _resolved_mask(cols, name, clause):
    """The docs a clause dict allows by way of the resolver's records and the restatement"""
    res = WhereResolver(cols)
    cid = res.clause({"field": name, **clause})
    n = len(cols[name])
    if cid < 0:
        return np.zeros(n, dtype=bool), res
    rec, values, _ = res.arrays([((cid,), (), ())])
    rcols = [(cols[c].type, cols[c].data, cols[c].valid) for c in res.names]
    return fields_ref.clause_holds(rcols, fields_ref.records(rec)[cid], values, n), res


F32_VALUES = np.asarray([0.1, np.nextafter(np.float32(0.1), np.float32(0)), np.nextafter(np.float32(0.1), np.float32(1)), 0.0, -0.0, 1e-45, -1e-45,
                         np.inf, -np.inf, np.nan, 3.4028235e38, -3.4028235e38, 16777216.0, 16777218.0, 0.5, -0.5, 1.0, 2.0], dtype=np.float32)
F32_BOUNDS = [0.1, -0.1, 0.30000000000000004, 1e-46, -1e-46, 1e39, -1e39, 16777217, 16777217.0, 2 ** 200, -(2 ** 200), 10 ** 400, 0, 0.0, -0.0, 0.5, 1,
              math.inf, -math.inf, math.nan, float(np.float32(0.1)), 3.4028235e38, 3.4028236e38]


@pytest.mark.parametrize("key", ["gte", "gt", "lte", "lt", "eq"])
def test_float_bounds_are_exact(key):
    cols = host_columns({"x": F32_VALUES})
    assert cols["x"].kind == "float32"
    for b in F32_BOUNDS:
        got, _ = _resolved_mask(cols, "x", {key: b})
        exp = fields_ref.where_mask(list(F32_VALUES), {key: b})
        assert np.array_equal(got, exp), (key, b, got.tolist(), exp.tolist())
    # spot checks by hand: 0.1 is no float32, so gte 0.1 starts at the float32 above it and lte 0.1 ends at the one below
    up, down = float(np.nextafter(np.float32(0.1), np.float32(1))), float(np.nextafter(np.float32(0.1), np.float32(0)))
    assert float(np.float32(0.1)) > 0.1 and down < 0.1
    assert fields.f32_at_least(0.1) == np.float32(0.1) and fields.f32_at_most(0.1) == np.float32(down)
    assert fields.f32_at_least(float(np.float32(0.1))) == np.float32(0.1) and up > 0.1
    assert fields.f32_at_least(math.nan) is None and fields.f32_at_most(10 ** 400) == np.float32(3.4028235e38)


def test_float_combined_in_and_exists():
    cols = host_columns({"x": F32_VALUES})
    for clause in ({"gte": 0.1, "lt": 2}, {"gt": -0.5, "lte": 0.5}, {"gt": 0.5, "lt": 0.5}, {"gte": 2, "lte": 1}, {"gte": -math.inf, "lte": math.inf},
                   {"in": [0.1, 0.5, 7, math.nan, 16777217, 10 ** 400]}, {"in": [0, 1]}, {"in": []}, {"in": [0.1]}, {"exists": True}):
        got, _ = _resolved_mask(cols, "x", clause)
        assert np.array_equal(got, fields_ref.where_mask(list(F32_VALUES), clause)), clause
    got, _ = _resolved_mask(cols, "x", {"exists": True})
    assert got.sum() == len(F32_VALUES) - 1 and not got[9]  # the NaN counts as missing


INT_BOUNDS = [0, -1, 1, 2.5, -2.5, 2.0, 0.999999, I32_MIN, I32_MAX, I32_MIN - 1, I32_MAX + 1, I64_MIN, I64_MAX, I64_MIN - 1, I64_MAX + 1, 2 ** 33, -(2 ** 33),
              2 ** 33 + 0.5, 9.3e18, -9.3e18, 1e300, -1e300, math.inf, -math.inf, math.nan, 10 ** 30, True]


@pytest.mark.parametrize("kind", ["int32", "int64"])
@pytest.mark.parametrize("key", ["gte", "gt", "lte", "lt", "eq"])
def test_int_bounds_are_exact(kind, key):
    if kind == "int32":
        data = np.asarray([I32_MIN, I32_MIN + 1, -3, -2, -1, 0, 1, 2, 3, I32_MAX - 1, I32_MAX], dtype=np.int32)
    else:
        data = np.asarray([I64_MIN, I64_MIN + 1, I32_MIN - 1, I32_MIN, -3, -2, -1, 0, 1, 2, 3, I32_MAX, I32_MAX + 1, 2 ** 33, 2 ** 33 + 1, -(2 ** 33), I64_MAX - 1,
                           I64_MAX], dtype=np.int64)
    cols = host_columns({"x": data})
    assert cols["x"].kind == kind
    for b in INT_BOUNDS:
        got, _ = _resolved_mask(cols, "x", {key: b})
        exp = fields_ref.where_mask([int(v) for v in data], {key: b})
        assert np.array_equal(got, exp), (kind, key, b, got.tolist(), exp.tolist())
    for clause in ({"gte": -2, "lt": 2.5}, {"gt": 2, "lt": 3}, {"in": [1, 2.0, 2.5, 10 ** 30, -3, I64_MAX, I32_MAX]}, {"in": [2.5]}, {"exists": True}):
        got, _ = _resolved_mask(cols, "x", clause)
        assert np.array_equal(got, fields_ref.where_mask([int(v) for v in data], clause)), (kind, clause)
    # a bound beyond the column's range is clamped or makes the clause unsatisfiable: nothing wraps
    res = WhereResolver(cols)
    big = I32_MAX + 1 if kind == "int32" else I64_MAX + 1
    assert res.clause({"field": "x", "gte": big}) == -1 and res.clause({"field": "x", "lt": -big}) == -1 and res.clause({"field": "x", "eq": big}) == -1
    c = res.clause({"field": "x", "lte": big})
    assert res.clauses[c][3] == big - 1 and res.clauses[c][2] == -big


def test_categories_sets_bools_and_missing():
    src = ["wiki", "arxiv", None, "web", "wiki", "news", None, "arxiv"]
    tags = [{"a", "b"}, ["b"], None, (), {"c"}, {"a", "c", "b"}, ["d", "d"], set()]
    flag = [True, False, None, True, False, False, True, None]
    cnt = [3, None, 5, 2 ** 40, -1, 0, 7, 8]
    cols = host_columns({"src": src, "tags": tags, "flag": flag, "cnt": cnt})
    assert [cols[k].kind for k in ("src", "tags", "flag", "cnt")] == ["category", "set", "bool", "int64"]
    assert cols["src"].dictionary == ["arxiv", "news", "web", "wiki"] and cols["src"].data.dtype == np.int32
    assert cols["src"].data.tolist() == [3, 0, 0, 2, 3, 1, 0, 0] and cols["src"].valid.tolist() == [v is not None for v in src]
    assert cols["tags"].dictionary == ["a", "b", "c", "d"] and cols["tags"].data.tolist() == [3, 2, 0, 0, 4, 7, 8, 0] and cols["tags"].type == 3
    assert cols["flag"].data.tolist() == [1, 0, 0, 1, 0, 0, 1, 0] and cols["flag"].type == 0
    cases = [("src", {"eq": "wiki"}), ("src", {"eq": "blog"}), ("src", {"in": ["wiki", "blog", "arxiv"]}), ("src", {"in": ["blog"]}), ("src", {"exists": True}),
             ("tags", {"any_of": ["a", "zz"]}), ("tags", {"any_of": ["zz"]}), ("tags", {"all_of": ["a", "b"]}), ("tags", {"all_of": ["a", "zz"]}),
             ("tags", {"all_of": []}), ("tags", {"any_of": []}), ("tags", {"exists": True}), ("flag", {"eq": True}), ("flag", {"eq": 0}),
             ("flag", {"exists": True}), ("cnt", {"gte": 5}), ("cnt", {"eq": 2 ** 40}), ("cnt", {"in": [3, 8, 2 ** 40]})]
    raw = {"src": src, "tags": tags, "flag": flag, "cnt": cnt}
    for name, clause in cases:
        got, _ = _resolved_mask(cols, name, clause)
        assert np.array_equal(got, fields_ref.where_mask(raw[name], clause)), (name, clause, got.tolist())
    res = WhereResolver(cols)
    assert res.clause({"field": "src", "eq": "blog"}) == -1            # an unknown category
    assert res.clause({"field": "tags", "all_of": ["a", "zz"]}) == -1  # all_of with an unknown label
    assert res.clause({"field": "tags", "any_of": ["zz"]}) == -1
    c = res.clause({"field": "src", "in": ["wiki", "blog", "arxiv"]})  # the unknown one is dropped from the list
    assert res.clauses[c][1] == fields_ref.IN and res.clauses[c][2] == (0, 3)
    # tests that do not fit the column, and malformed clauses
    for bad in ({"field": "src", "gte": "a"}, {"field": "src", "any_of": ["a"]}, {"field": "tags", "eq": "a"}, {"field": "tags", "gte": 1},
                {"field": "cnt", "all_of": ["a"]}, {"field": "cnt", "eq": "3"}, {"field": "nope", "eq": 1}, {"field": "cnt"}, {"field": "cnt", "eq": 1, "gte": 0},
                {"field": "cnt", "near": 1}, {"field": "cnt", "exists": False}, {"eq": 1}, "cnt", {"field": "tags", "any_of": "a"}, {"field": "src", "eq": 3},
                {"field": "cnt", "in": 3}):
        with pytest.raises(ValueError):
            WhereResolver(cols).clause(bad)
    # numpy.ma: masked entries are the validity row
    ma = np.ma.masked_array(np.asarray([1.5, 2.5, 3.5], np.float32), mask=[False, True, False])
    c = host_column("p", ma)
    assert c.kind == "float32" and c.valid.tolist() == [True, False, True]
    assert host_column("p", np.ma.masked_array(np.asarray([1, 2], np.int32), mask=False)).valid is None


def test_column_refusals():
    with pytest.raises(ValueError, match="cast it to float32"):
        host_column("x", np.asarray([1.0, 2.0]))
    with pytest.raises(ValueError, match="cast it to float32"):
        host_column("x", [1.5, None, 2.0])
    with pytest.raises(ValueError, match="cast it to float32"):
        host_column("x", np.ma.masked_array([1.0, 2.0], mask=[0, 1]))
    labels = [f"l{i:02d}" for i in range(65)]
    assert host_column("t", [labels[:64], None]).data[0] == -1  # 64 labels: every bit, bit 63 included
    with pytest.raises(ValueError, match="65 distinct labels"):
        host_column("t", [labels[:40], labels[40:]])
    for bad in ([None, None], "abc", [1, "a"], [[1, 2]], np.zeros((2, 2), np.int32), np.asarray([1 + 2j]), 5):
        with pytest.raises(ValueError):
            host_column("x", bad)
    with pytest.raises(ValueError, match="lengths differ"):
        host_columns({"a": [1, 2], "b": [1, 2, 3]})
    for bad in ({}, None, [1, 2]):
        with pytest.raises(ValueError):
            host_columns(bad)
    assert host_column("x", np.asarray([1, 2], np.uint8)).kind == "int32" and host_column("x", np.asarray([1, 2 ** 32 - 1], np.uint32)).kind == "int64"


def test_groups_share_clauses_and_rows():
    cols = host_columns({"year": np.arange(10, dtype=np.int32), "src": ["a", "b"] * 5, "tags": [["x"], ["y"]] * 5})
    res = WhereResolver(cols, share_rows=True)
    g1 = {"must": [{"field": "year", "gte": 3}, {"field": "src", "in": ["a", "zz"]}], "must_not": [{"field": "tags", "any_of": ["y"]}]}
    g2 = [{"field": "year", "gte": 3.0}, {"field": "year", "gt": 2}]  # a bare list is must; both clauses resolve to the record of g1's first
    assert res.add(g1) == 0 and res.add(g2) == 1 and res.add(dict(g1)) == 0 and res.add({"must": list(g2)}) == 1
    assert res.add({}) == -1 and res.add([]) == -1 and res.add({"should": []}) == -1
    assert res.add({"field": "year", "gte": 3}) == 2  # one clause dict is a must of one
    assert res.names == ["year", "src", "tags"] and len(res.clauses) == 3
    assert res.rows == [((0, 1), (), (2,)), ((0, 0), (), ()), ((0,), (), ())]
    assert res.add({"should": [{"field": "src", "eq": "zz"}]}) == 3 and res.rows[3] == ((), (-1,), ())
    rec, values, lists = res.arrays()
    assert rec.dtype == np.int64 and rec.shape == (3, 3) and values.tolist() == []  # an in of one known value is a range
    assert fields_ref.records(rec)[0] == (0, fields_ref.RANGE, 3, I32_MAX)
    assert [p.tolist() for p, _ in lists] == [[0, 2, 4, 5, 5], [0, 0, 0, 0, 1], [0, 1, 1, 1, 1]]
    assert [c.tolist() for _, c in lists] == [[0, 1, 0, 0, 0], [-1], [2]]
    fields.check_records([cols[n].type for n in res.names], rec, len(values), lists)
    # without sharing every group is a row, the empty one too
    res = WhereResolver(cols)
    assert [res.add(g) for g in (g1, g1, {})] == [0, 1, 2] and res.rows[2] == ((), (), ())
    for bad in ({"must": {"field": "year", "eq": 1}}, {"filter": []}, 7, "year", {"must": "x"}):
        with pytest.raises(ValueError):
            WhereResolver(cols).add(bad)
    assert fields.where_groups(g1) == [g1] and fields.where_groups(g2) == [g2] and fields.where_groups([g1, g2]) == [g1, g2]
    assert fields.where_groups([g2, []]) == [g2, []]
    assert fields.where_groups([]) == [[]]  # the empty list is the empty group: one row that constrains nothing
    for bad in (None, 3, "year"):
        with pytest.raises(ValueError):
            fields.where_groups(bad)


def test_check_records():
    types = [fields_ref.I32, fields_ref.SET64, fields_ref.F32]
    rec = lambda *rows: np.asarray([[c | (op << 32), lo, hi] for c, op, lo, hi in rows], dtype=np.int64).reshape(-1, 3)
    lists = lambda ids, n=1: [(np.asarray([0] + [len(ids)] * n, np.int32), np.asarray(ids, np.int32)), None, None]
    good = rec((0, 0, 1, 5), (1, 2, 7, 0), (1, 3, 7, 0), (2, 1, 1, 2), (0, 1, 0, 3))
    fields.check_records(types, good, 3, lists([0, 1, 2, 3, 4, -1]))
    for bad_rec, n_values, ids in ((rec((3, 0, 0, 0)), 0, [0]), (rec((0, 2, 1, 0)), 0, [0]), (rec((1, 0, 0, 1)), 0, [0]), (rec((2, 3, 0, 0)), 0, [0]),
                                   (rec((0, 4, 0, 0)), 0, [0]), (rec((0, 1, 2, 2)), 3, [0]), (rec((0, 1, -1, 1)), 3, [0]), (rec((0, 1, 0, -1)), 3, [0]),
                                   (good, 3, [5]), (good, 3, [-2])):
        with pytest.raises(ValueError):
            fields.check_records(types, bad_rec, n_values, lists(ids))
    with pytest.raises(ValueError):
        fields.check_records(types, good, 3, [None, None, None])
    with pytest.raises(ValueError):
        fields.check_records(types, good, 3, [lists([0])[0], lists([0, 0], 2)[0], None])
    with pytest.raises(ValueError):
        fields.check_records(types, good.astype(np.int32), 3, lists([0]))


def test_columns_from_metadata():
    corpus = {"d0": {"text": "a", "metadata": {"year": 2020, "src": "wiki", "tags": ["x"]}}, "d1": {"text": "b"}, "d2": {"text": "c", "metadata": None},
              "d3": {"text": "d", "metadata": {"year": 2024, "extra": 1}}}
    cols = sparse_rx.columns_from_metadata(corpus, ["year", "src", "tags", "absent"])
    assert cols == {"year": [2020, None, None, 2024], "src": ["wiki", None, None, None], "tags": [["x"], None, None, None], "absent": [None] * 4}
    assert list(cols) == ["year", "src", "tags", "absent"]
    h = host_columns({k: v for k, v in cols.items() if k != "absent"})
    assert h["year"].kind == "int64" and h["year"].valid.tolist() == [True, False, False, True] and h["tags"].kind == "set"
    with pytest.raises(ValueError):
        sparse_rx.columns_from_metadata(corpus, "year")


# ---- the keyword of the API mirrors ---------------------------------------------------------------------------------------------
QUERIES = {"a": "x", "b": "y", "c": "z"}
SCHEMA = host_columns({"year": np.arange(2000, 2010, dtype=np.int32), "src": ["wiki", "web"] * 5})
G1 = {"must": [{"field": "year", "gte": 2005}]}
G2 = [{"field": "src", "eq": "wiki"}]


def test_field_filter_spec():
    s = field_filter_spec(SCHEMA, QUERIES, G1)
    assert isinstance(s, FieldFilterSpec) and s.rows == [((0,), (), ())] and s.row_of_qid == {"a": 0, "b": 0, "c": 0}
    assert field_filter_spec(SCHEMA, QUERIES, {}) is None and field_filter_spec(SCHEMA, QUERIES, []) is None
    assert field_filter_spec(SCHEMA, QUERIES, {"other": G1}) is None and field_filter_spec(SCHEMA, QUERIES, {"a": {}}) is None
    s = field_filter_spec(SCHEMA, QUERIES, G2)  # a bare list of clauses is one group for every query
    assert s.rows == [((0,), (), ())] and s.resolver.names == ["src"]
    # the dict form: a qid missing from it is not constrained; equal groups share a row, equal clauses a record
    s = field_filter_spec(SCHEMA, QUERIES, {"a": G1, "c": {"must": [{"field": "year", "gt": 2004}]}, "zz": G2})
    assert s.rows == [((0,), (), ())] and s.row_of_qid == {"a": 0, "b": -1, "c": 0} and len(s.resolver.clauses) == 1
    s = field_filter_spec(SCHEMA, QUERIES, {"a": G1, "b": G2, "c": {"must": G1["must"], "must_not": G2}})
    assert s.rows == [((0,), (), ()), ((1,), (), ()), ((0,), (), (1,))] and s.row_of_qid == {"a": 0, "b": 1, "c": 2}
    # a dict whose keys all lie in {must, should, must_not} is a group, whatever the qids are called
    s = field_filter_spec(SCHEMA, {"must": "x", "b": "y"}, {"must": [{"field": "year", "eq": 2001}]})
    assert s.row_of_qid == {"must": 0, "b": 0}
    for bad in (7, "year", {"a": 7}, {"a": {"must": [{"field": "nope", "eq": 1}]}}, {"must": [{"field": "src", "gte": 1}]}):
        with pytest.raises(ValueError):
            field_filter_spec(SCHEMA, QUERIES, bad)


def test_field_spec_with_doc_and_term_bases():
    row_of = {f"d{i}": i for i in range(10)}
    flds = field_filter_spec(SCHEMA, QUERIES, {"a": G1, "b": G1})
    assert flds.with_base(None, QUERIES) is flds
    docs = doc_filter_spec(row_of, QUERIES, {"b": ["d1"], "c": ["d2", "d3"]}, None)
    s = flds.with_base(docs, QUERIES)
    # distinct (doc row, field row) pairs: a = (-1, 0), b = (0, 0), c = (1, -1)
    assert s.base is docs and s.row_of_qid == {"a": 0, "b": 1, "c": 2} and s.resolver is flds.resolver
    assert s.rows == [((0,), (), ()), ((0,), (), ()), ((), (), ())] and s.base_rows == [-1, 0, 1]
    docs = doc_filter_spec(row_of, QUERIES, None, ["d5"])  # one list for every query: a and b share (0, 0)
    s = flds.with_base(docs, QUERIES)
    assert s.row_of_qid == {"a": 0, "b": 0, "c": 1} and s.base_rows == [0, 0] and s.rows == [((0,), (), ()), ((), (), ())]
    # the chain doc filter -> term rows -> field rows: the term spec, itself over the doc spec, is the base
    terms = term_filter_spec({"gpu": 0}, QUERIES, {"a": ["gpu"], "c": ["gpu"]}).with_base(docs, QUERIES)
    assert terms.row_of_qid == {"a": 0, "b": 1, "c": 0}
    s = flds.with_base(terms, QUERIES)
    assert s.base is terms and s.base.base is docs and s.row_of_qid == {"a": 0, "b": 1, "c": 2} and s.base_rows == [0, 1, 0]
    assert s.rows == [((0,), (), ()), ((0,), (), ()), ((), (), ())]
    with pytest.raises(ValueError, match="field table"):
        s.on_device(None)


# ---- the mirrors with no keyword given, the sharded refusal and the no-fields refusal ------------------------------------------------
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


def test_mirrors_unchanged_without_keyword_and_refusals(golden_dir, one_rank_group, tmp_path):
    """The fake backend of test_dict_search_cpu.py (the CPU oracle behind the sharding protocol, counting its searches): a call
    without ``where`` searches and caches as before; with it, a backend without fields and a sharded backend refuse before they search."""
    from test_dict_search_cpu import _Counted
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    q = {qid: j["queries"][qid] for qid in ("q0", "q1", "q2")}
    n = len(j["corpus"])
    where = {"must": [{"field": "year", "gte": 2010}]}
    for make, method in ((lambda f: sparse_rx.RetrievalService(shard_searcher_factory=f, sharded=True), "search_bm25"),
                         (lambda f: sparse_rx.OptimizedBM25Retriever(shard_searcher_factory=f, sharded=True), "search"),
                         (lambda f: sparse_rx.OptimizedRetriever({"type": "bm25"}, shard_searcher_factory=f, sharded=True, cache_dir=str(tmp_path)), "search")):
        f = _Counted()
        o = make(f)
        with pytest.raises(ValueError, match="not built"):
            o.set_doc_fields({"year": np.arange(n, dtype=np.int32)})
        (o.build_bm25_index if method == "search_bm25" else o.build_index_from_corpus)(j["corpus"])
        search = getattr(o, method)
        r = search(q, top_k=10)
        assert f.take() == [(3, 10)] and len(o.query_cache) == 3 and all(r[qid] for qid in q)
        assert search(q, top_k=10, where=None) == r and f.take() == []  # the keyword at its default: the same dicts, from the cache
        # where= without set_doc_fields: a ValueError that names the call
        with pytest.raises(ValueError, match=rf"{method}\(where=\.\.\.\) needs the docs' fields: call set_doc_fields"):
            search(q, top_k=10, where=where)
        with pytest.raises(ValueError, match="one entry per doc"):
            o.set_doc_fields({"year": np.arange(n + 1, dtype=np.int32)})
        with pytest.raises(ValueError, match="cast it to float32"):
            o.set_doc_fields({"price": np.ones(n)})
        o.set_doc_fields({"year": np.arange(2000, 2000 + n, dtype=np.int32)})
        assert search(q, top_k=10) == r and search(q, top_k=10, where={}) == r and search(q, top_k=10, where={"zz": where}) == r and f.take() == []
        for kw in (dict(where=where), dict(where={"q0": where}), dict(where=where, excluded_docs=[next(iter(j["corpus"]))]), dict(where=where, must_terms=["w3"])):
            with pytest.raises(ValueError, match="whole index on one GPU"):
                search(q, top_k=10, **kw)
        with pytest.raises(ValueError, match="unknown field"):
            search(q, top_k=10, where=[{"field": "nope", "eq": 1}])
        assert f.take() == [] and len(o.query_cache) == 3
        o.close()


def test_service_doors_before_any_device():
    svc = sparse_rx.RetrievalService(device="cuda:0")
    with pytest.raises(ValueError, match="one group"):  # checked before the index is looked at
        svc.search_by_vector(np.zeros(4, np.float32), where={"q": {"must": []}})
    with pytest.raises(ValueError, match="not built"):
        svc.set_doc_fields({"year": [1, 2]})
    for cls in (sparse_rx.HybridRetriever, sparse_rx.ShardedSearcher, sparse_rx.HostBatchPipeline):
        assert not hasattr(cls, "set_doc_fields")
    import inspect
    assert "where" not in inspect.signature(sparse_rx.HybridRetriever.search).parameters
    for fn in (sparse_rx.RetrievalService.search_bm25, sparse_rx.RetrievalService.search_by_vector, sparse_rx.RetrievalService.search_hybrid,
               sparse_rx.OptimizedBM25Retriever.search, sparse_rx.OptimizedRetriever.search):
        p = inspect.signature(fn).parameters["where"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
