"""Field predicates (include/sparse_rx_fields.h): doc metadata as resident columns, and predicates over them as filter rows.

A :class:`FieldTable` keeps typed columns of a corpus on the GPU -- int32 / int64 / float32 values, categories (strings as
int32 codes, the dictionary stays on the host) and label sets (up to 64 labels as the bits of an int64) -- each with an optional
validity row for the docs that have no value.  :meth:`FieldTable.filter` turns a ``where`` predicate into the rows of a
:class:`~.filter.DocFilter` (``srx_filter_from_fields``), which every filtered search takes as it is.  The reference has no
filters, and nothing reads its ``metadata`` dicts: nothing here mirrors reference code.

The predicate is resolved to clause records ON THE HOST (:class:`WhereResolver`), so that the device's same-type comparison
equals the comparison in exact arithmetic: a Python bound on a float32 column is rounded towards the inside of its range, a
non-integral or out-of-range bound on an integer column likewise, and what no value can satisfy becomes clause id -1.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi
from .filter import BASE_NAMES, DocFilter, build_rows, filter_words, host_q_filter, pack_masks, q_filter_to_device

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
GROUP_KEYS = ("must", "should", "must_not")
NULL_POLICIES = {"own": _capi.SRX_COLLAPSE_NULL_OWN, "one": _capi.SRX_COLLAPSE_NULL_ONE, "drop": _capi.SRX_COLLAPSE_NULL_DROP}
ORDERS = {"asc": _capi.SRX_ORDER_ASC, "desc": _capi.SRX_ORDER_DESC}
ORDER_NULLS = {"last": _capi.SRX_ORDER_NULLS_LAST, "first": _capi.SRX_ORDER_NULLS_FIRST, "drop": _capi.SRX_ORDER_NULLS_DROP}
_RANGE_KEYS = ("gte", "gt", "lte", "lt")
_TEST_KEYS = _RANGE_KEYS + ("eq", "in", "any_of", "all_of", "exists")


def _torch():
    import torch
    return torch


_ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # what a C entry point takes for an optional or empty tensor


class HostColumn:
    """One column on the host: ``kind`` ("int32", "int64", "float32", "bool", "category", "set"), ``type`` (its SRX_FIELD_*),
    ``data`` (the array that goes to the device: int32 / int64 / float32; int64 holds a set's bits), ``valid`` (bool[n_docs],
    or None when every doc has a value) and ``dictionary`` (the sorted distinct strings of a category column -- code = position
    --, the labels of a set column -- label i = bit i --, else None)."""

    def __init__(self, kind: str, data: np.ndarray, valid: Optional[np.ndarray], dictionary=None):
        self.kind, self.data, self.valid, self.dictionary = kind, np.ascontiguousarray(data), valid, dictionary
        self.type = {"int32": _capi.SRX_FIELD_I32, "bool": _capi.SRX_FIELD_I32, "category": _capi.SRX_FIELD_I32, "int64": _capi.SRX_FIELD_I64,
                     "float32": _capi.SRX_FIELD_F32, "set": _capi.SRX_FIELD_SET64}[kind]
        self.code_of = {s: i for i, s in enumerate(dictionary)} if dictionary is not None else None

    def __len__(self) -> int:
        return int(self.data.shape[0])


def _array_column(name: str, a: np.ndarray, valid) -> HostColumn:
    if a.ndim != 1:
        raise ValueError(f"column {name!r} must have one entry per doc (a 1-D sequence)")
    if a.dtype == np.float64:
        raise ValueError(f"column {name!r} is float64: cast it to float32 (the device compares float32 values; a float64 column would "
                         "change the values a bound is compared with)")
    if a.dtype == np.bool_:
        return HostColumn("bool", a.astype(np.int32), valid)
    if a.dtype in (np.int8, np.int16, np.uint8, np.uint16):
        a = a.astype(np.int32)
    elif a.dtype == np.uint32:
        a = a.astype(np.int64)
    if a.dtype == np.int32:
        return HostColumn("int32", a, valid)
    if a.dtype == np.int64:
        return HostColumn("int64", a, valid)
    if a.dtype == np.float32:
        return HostColumn("float32", a, valid)
    raise ValueError(f"column {name!r} has dtype {a.dtype}: give int32, int64, float32 or bool values, strings or collections of strings")


def host_column(name: str, values) -> HostColumn:
    """One entry of ``columns`` as a :class:`HostColumn` (the type mapping of :meth:`FieldTable.from_columns`)"""
    if isinstance(values, np.ma.MaskedArray):
        mask = np.ma.getmaskarray(values)
        valid = None if not mask.any() else ~mask
        data = np.asarray(values.filled(0) if values.dtype != np.bool_ else values.filled(False))
        return _array_column(name, data, valid)
    if isinstance(values, np.ndarray) and values.dtype != object:
        if values.dtype.kind in "US":
            values = values.tolist()
        else:
            return _array_column(name, values, None)
    if isinstance(values, (str, bytes)) or not hasattr(values, "__len__"):
        raise ValueError(f"column {name!r} must be a sequence with one entry per doc")
    seq = list(values)
    valid = np.asarray([v is not None for v in seq], dtype=bool)
    some = [v for v in seq if v is not None]
    if not some:
        raise ValueError(f"column {name!r} holds no value at all: its type cannot be told")
    valid_or_none = None if valid.all() else valid
    if all(isinstance(v, str) for v in some):
        dictionary = sorted(set(some))
        code = {s: i for i, s in enumerate(dictionary)}
        return HostColumn("category", np.asarray([code[v] if v is not None else 0 for v in seq], dtype=np.int32), valid_or_none, dictionary)
    if all(isinstance(v, (set, frozenset, list, tuple)) for v in some):
        if not all(isinstance(s, str) for v in some for s in v):
            raise ValueError(f"column {name!r}: a set column holds collections of strings")
        labels = sorted({s for v in some for s in v})
        if len(labels) > 64:
            raise ValueError(f"column {name!r} holds {len(labels)} distinct labels: a set column takes at most 64")
        bit = {s: i for i, s in enumerate(labels)}
        bits = np.asarray([sum(1 << bit[s] for s in set(v)) if v is not None else 0 for v in seq], dtype=np.uint64)
        return HostColumn("set", bits.view(np.int64), valid_or_none, labels)
    if all(isinstance(v, (bool, np.bool_)) for v in some):
        return HostColumn("bool", np.asarray([int(bool(v)) if v is not None else 0 for v in seq], dtype=np.int32), valid_or_none)
    if all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in some):
        if any(not (I64_MIN <= int(v) <= I64_MAX) for v in some):
            raise ValueError(f"column {name!r} holds an integer outside int64")
        return HostColumn("int64", np.asarray([int(v) if v is not None else 0 for v in seq], dtype=np.int64), valid_or_none)
    if all(isinstance(v, np.float32) for v in some):
        return HostColumn("float32", np.asarray([v if v is not None else 0 for v in seq], dtype=np.float32), valid_or_none)
    if all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) for v in some):
        raise ValueError(f"column {name!r} holds Python / float64 numbers: cast it to float32 (a float32 array, or a numpy.ma array of "
                         "float32 where entries are missing)")
    raise ValueError(f"column {name!r} mixes value types: give numbers, strings or collections of strings (None = no value)")


def host_columns(columns) -> Dict[str, HostColumn]:
    """``columns`` (name -> sequence of n_docs entries) as :class:`HostColumn` objects; the lengths must agree."""
    if not isinstance(columns, dict) or not columns:
        raise ValueError("columns must be a non-empty dict name -> sequence of n_docs entries")
    out = {str(name): host_column(str(name), values) for name, values in columns.items()}
    if len({len(c) for c in out.values()}) != 1:
        raise ValueError("the columns must have one entry per doc each: their lengths differ")
    if len(next(iter(out.values()))) < 1:
        raise ValueError("the columns are empty")
    return out


def columns_from_metadata(corpus, names: Sequence[str]) -> Dict[str, list]:
    """The ``metadata`` dicts of a corpus (``{doc_id: {"text": ..., "metadata": {...}}}``) as columns in the corpus's order:
    ``{name: [corpus[doc_id].get("metadata") or {} ).get(name) for every doc]}``; a missing key is None."""
    if isinstance(names, (str, bytes)):
        raise ValueError("names must be a sequence of field names, not one string")
    metas = [(doc.get("metadata") or {}) if isinstance(doc, dict) else {} for doc in corpus.values()]
    return {name: [m.get(name) for m in metas] for name in names}


# ---- exact bounds -------------------------------------------------------------------------------------------------------------
def _number(x, what):
    if isinstance(x, (bool, np.bool_)):
        return int(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    raise ValueError(f"{what} must be a number, got {x!r}")


def _f32_nearest(b) -> np.float32:
    try:
        with np.errstate(over="ignore"):
            return np.float32(float(b))
    except OverflowError:  # an int beyond float64
        return np.float32(np.inf if b > 0 else -np.inf)


def f32_at_least(b):
    """The smallest float32 >= b in exact arithmetic (b an int or a float; NaN: None)"""
    if isinstance(b, float) and math.isnan(b):
        return None
    f = _f32_nearest(b)
    if float(f) < b:  # Python compares an int with a float exactly
        with np.errstate(over="ignore"):
            f = np.nextafter(f, np.float32(np.inf))
    return f


def f32_at_most(b):
    """The largest float32 <= b in exact arithmetic (NaN: None)"""
    if isinstance(b, float) and math.isnan(b):
        return None
    f = _f32_nearest(b)
    if float(f) > b:
        with np.errstate(over="ignore"):
            f = np.nextafter(f, np.float32(-np.inf))
    return f


def f32_bits(f) -> int:
    """The bits of a float32 as a non-negative int (the low 32 bits of a clause's lo / hi or of a ``values`` entry)"""
    return int(np.asarray(f, dtype=np.float32).view(np.uint32))


def _int_floor(b):
    return b if isinstance(b, int) else None if math.isnan(b) else I64_MAX + 1 if b == math.inf else I64_MIN - 1 if b == -math.inf else math.floor(b)


def _int_ceil(b):
    return b if isinstance(b, int) else None if math.isnan(b) else I64_MAX + 1 if b == math.inf else I64_MIN - 1 if b == -math.inf else math.ceil(b)


class WhereResolver:
    """``where`` groups -> clause records, over the columns of one table (``schema``: name -> :class:`HostColumn` or anything with
    its ``kind`` / ``type`` / ``code_of``).  Equal clauses share a record, and with ``share_rows`` equal groups share a row.

    ``names``    the columns the clauses name, in the order of first use: a clause's ``col`` indexes this list
    ``clauses``  [(col, op, lo, hi)]; an IN clause holds its value tuple in ``lo`` until :meth:`arrays` lays the lists out
    ``rows``     [(all, any, none)] tuples of clause ids, -1 = a clause no doc satisfies"""

    def __init__(self, schema, share_rows: bool = False):
        self.schema, self.share_rows = schema, share_rows
        self.names: List[str] = []
        self.clauses: List[tuple] = []
        self.rows: List[tuple] = []
        self._clause_of, self._row_of = {}, {}

    # -- one clause ---------------------------------------------------------------------------------------------------------
    def _record(self, name, op, lo, hi) -> int:
        key = (name, op, lo, hi)
        if key not in self._clause_of:
            if name not in self.names:
                self.names.append(name)
            self._clause_of[key] = len(self.clauses)
            self.clauses.append((self.names.index(name), op, lo, hi))
        return self._clause_of[key]

    def clause(self, c) -> int:
        """One clause dict -> its record's id, or -1 when no value can satisfy it.  Raises ValueError for a malformed clause, an
        unknown field and a test that does not fit the column's type."""
        if not isinstance(c, dict) or "field" not in c:
            raise ValueError(f"a clause is a dict with \"field\" and a test, got {c!r}")
        name = c["field"]
        if name not in self.schema:
            raise ValueError(f"unknown field {name!r}")
        tests = [k for k in c if k != "field"]
        if not tests or any(k not in _TEST_KEYS for k in tests):
            raise ValueError(f"the clause on {name!r} needs one of {', '.join(_TEST_KEYS)}; got {sorted(tests)}")
        if len(tests) > 1 and any(k not in _RANGE_KEYS for k in tests):
            raise ValueError(f"the clause on {name!r} combines {sorted(tests)}: only gte / gt / lte / lt combine")
        col = self.schema[name]
        kind = col.kind
        if "exists" in c:
            if c["exists"] is not True:
                raise ValueError("exists takes True only: put the clause under must_not for the docs without a value")
            if kind == "set":
                return self._record(name, _capi.SRX_FOP_MASK_ALL, 0, 0)
            if kind == "float32":  # the full range: a NaN passes no range, so it counts as missing
                return self._record(name, _capi.SRX_FOP_RANGE, f32_bits(-np.inf), f32_bits(np.inf))
            lo, hi = (I64_MIN, I64_MAX) if kind == "int64" else (I32_MIN, I32_MAX)
            return self._record(name, _capi.SRX_FOP_RANGE, lo, hi)
        if "any_of" in c or "all_of" in c:
            key = "any_of" if "any_of" in c else "all_of"
            if kind != "set":
                raise ValueError(f"{key} is for set columns; {name!r} is a {kind} column")
            labels = c[key]
            if isinstance(labels, (str, bytes)) or not hasattr(labels, "__iter__"):
                raise ValueError(f"{key} takes a collection of labels, not {labels!r}")
            labels = list(labels)
            known = [col.code_of[s] for s in labels if s in col.code_of]
            mask = sum(1 << b for b in set(known))
            if key == "all_of":
                if len(known) != len(labels):
                    return -1  # a label no doc carries
                return self._record(name, _capi.SRX_FOP_MASK_ALL, _as_i64(mask), 0)
            return self._record(name, _capi.SRX_FOP_MASK_ANY, _as_i64(mask), 0) if mask else -1
        if kind == "set":
            raise ValueError(f"{name!r} is a set column: it takes any_of / all_of / exists, not {sorted(tests)}")
        if "eq" in c or "in" in c:
            if "in" in c and (isinstance(c["in"], (str, bytes)) or not hasattr(c["in"], "__iter__")):
                raise ValueError(f"in takes a collection of values, not {c['in']!r}")
            wanted = [c["eq"]] if "eq" in c else list(c["in"])
            vals = sorted({v for v in (self._exact_value(name, col, x) for x in wanted) if v is not None})
            if not vals:
                return -1
            if len(vals) == 1:  # one value is the range [v, v] (a float's too: IEEE compares, so +0 takes -0 as == does)
                return self._record(name, _capi.SRX_FOP_RANGE, vals[0], vals[0])
            return self._record(name, _capi.SRX_FOP_IN, tuple(vals), len(vals))
        # ---- a range
        if kind == "category":
            raise ValueError(f"{name!r} is a category column: it takes eq / in / exists, not a range")
        bound = {k: _number(c[k], f"{k} on {name!r}") for k in tests}
        if kind == "float32":
            lo, hi = np.float32(-np.inf), np.float32(np.inf)
            for k, b in bound.items():
                if k in ("gte", "gt"):
                    f = f32_at_least(b)
                    if f is not None and k == "gt" and float(f) == b:
                        f = None if f == np.inf else np.nextafter(f, np.float32(np.inf))
                    if f is None:
                        return -1
                    lo = max(lo, f)
                else:
                    f = f32_at_most(b)
                    if f is not None and k == "lt" and float(f) == b:
                        f = None if f == -np.inf else np.nextafter(f, np.float32(-np.inf))
                    if f is None:
                        return -1
                    hi = min(hi, f)
            if lo > hi:
                return -1
            return self._record(name, _capi.SRX_FOP_RANGE, f32_bits(lo), f32_bits(hi))
        tmin, tmax = (I64_MIN, I64_MAX) if kind == "int64" else (I32_MIN, I32_MAX)
        lo, hi = tmin, tmax
        for k, b in bound.items():
            e = _int_ceil(b) if k in ("gte", "lt") else _int_floor(b)
            if e is None:  # NaN
                return -1
            if k == "gte":
                lo = max(lo, e)
            elif k == "gt":
                lo = max(lo, e + 1)
            elif k == "lte":
                hi = min(hi, e)
            else:
                hi = min(hi, e - 1)
        if lo > hi:  # also a bound beyond the column's range on the wrong side
            return -1
        return self._record(name, _capi.SRX_FOP_RANGE, lo, hi)

    def _exact_value(self, name, col, x):
        """What ``eq`` / ``in`` compare with, or None when no value of the column equals x"""
        kind = col.kind
        if kind == "category":
            if not isinstance(x, str):
                raise ValueError(f"{name!r} is a category column: it compares with strings, not {x!r}")
            return col.code_of.get(x)
        v = _number(x, f"a value for {name!r}")
        if kind == "float32":
            if isinstance(v, float) and math.isnan(v):
                return None
            f = _f32_nearest(v)
            if float(f) != v:
                return None
            return f32_bits(np.float32(0.0) if f == 0 else f)  # one spelling of zero: == takes both
        if isinstance(v, float):
            if not v.is_integer():
                return None
            v = int(v)
        tmin, tmax = (I64_MIN, I64_MAX) if kind == "int64" else (I32_MIN, I32_MAX)
        return v if tmin <= v <= tmax else None

    # -- groups -----------------------------------------------------------------------------------------------------------
    def group(self, g) -> tuple:
        """One group -> its (all, any, none) triple of clause ids"""
        g = as_group(g)
        return tuple(tuple(self.clause(c) for c in g.get(k, ())) for k in GROUP_KEYS)

    def add(self, g) -> int:
        """One group -> its row (-1 when the group holds no clause and rows are shared: nothing is constrained)"""
        triple = self.group(g)
        if not self.share_rows:
            self.rows.append(triple)
            return len(self.rows) - 1
        if triple == ((), (), ()):
            return -1
        if triple not in self._row_of:
            self._row_of[triple] = len(self.rows)
            self.rows.append(triple)
        return self._row_of[triple]

    def arrays(self, rows=None):
        """(clauses int64[n_clauses, 3], values int64[n_values], [(ptr, clause)] * 3) for ``rows`` (default: every row): a record
        is (col | op << 32, lo, hi), little-endian the 24 bytes of ``srx_field_clause``."""
        rows = self.rows if rows is None else rows
        rec = np.zeros((len(self.clauses), 3), dtype=np.int64)
        values: List[int] = []
        for i, (col, op, lo, hi) in enumerate(self.clauses):
            if op == _capi.SRX_FOP_IN:  # lo holds the value tuple
                first = len(values)
                values.extend(lo)
                lo = first
            rec[i] = (col | (op << 32), lo, hi)
        lists = []
        for which in range(3):
            ptr = np.zeros(len(rows) + 1, dtype=np.int32)
            ptr[1:] = np.cumsum([len(r[which]) for r in rows])
            lists.append((ptr, np.asarray([c for r in rows for c in r[which]], dtype=np.int32)))
        return rec, np.asarray(values, dtype=np.int64), lists


def _as_i64(mask: int) -> int:
    return mask - (1 << 64) if mask >= 1 << 63 else mask


def is_group(x) -> bool:
    """A dict whose keys all lie in {"must", "should", "must_not"} (the empty dict included), or a bare list of clause dicts"""
    if isinstance(x, dict):
        return all(k in GROUP_KEYS for k in x)
    return isinstance(x, (list, tuple)) and all(isinstance(c, dict) and "field" in c for c in x)


def as_group(g) -> dict:
    """A group in its dict form: a bare list of clauses is ``must``, one clause dict a ``must`` of one"""
    if isinstance(g, dict) and "field" in g:
        return {"must": [g]}
    if isinstance(g, dict):
        bad = [k for k in g if k not in GROUP_KEYS]
        if bad:
            raise ValueError(f"a group has the keys must / should / must_not, got {bad}")
        for k, v in g.items():
            if isinstance(v, dict) or isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
                raise ValueError(f"{k} takes a list of clauses, got {v!r}")
        return g
    if isinstance(g, (list, tuple)):
        return {"must": list(g)}
    raise ValueError(f"a group is a dict with must / should / must_not or a list of clauses, got {g!r}")


def where_groups(where) -> list:
    """``where`` of :meth:`FieldTable.filter` as a list of groups, one per output row: one group (a dict, or a bare list of
    clause dicts) is one row; any other list is a list of groups."""
    if isinstance(where, dict) or is_group(where):
        return [where]
    if isinstance(where, (list, tuple)) and len(where) > 0:
        return list(where)
    raise ValueError("where must be a group or a non-empty list of groups")


def check_records(types, clauses, n_values: int, lists) -> None:
    """What the device does not check of host arrays: every ``col`` in [0, len(types)), every op fit for its column's type, every
    IN range inside ``values``, every clause id in [-1, n_clauses).  Raises ValueError."""
    rec = np.asarray(clauses)
    if rec.ndim != 2 or rec.shape[1] != 3 or rec.dtype != np.int64:
        raise ValueError("clauses must be int64[n_clauses, 3]: (col | op << 32, lo, hi) per record")
    for i in range(rec.shape[0]):
        col, op, lo, hi = int(rec[i, 0] & 0xFFFFFFFF), int(rec[i, 0] >> 32), int(rec[i, 1]), int(rec[i, 2])
        if not (0 <= col < len(types)):
            raise ValueError(f"clause {i}: col {col} outside [0, {len(types)})")
        fits = (_capi.SRX_FOP_MASK_ANY, _capi.SRX_FOP_MASK_ALL) if types[col] == _capi.SRX_FIELD_SET64 else (_capi.SRX_FOP_RANGE, _capi.SRX_FOP_IN)
        if op not in fits:
            raise ValueError(f"clause {i}: op {op} does not fit a column of type {types[col]}")
        if op == _capi.SRX_FOP_IN and not (0 <= hi and 0 <= lo and lo + hi <= n_values):
            raise ValueError(f"clause {i}: its IN range [{lo}, {lo} + {hi}) lies outside the {n_values} values")
    n_rows = None
    for pair in lists:
        if pair is None:
            continue
        ptr, ids = np.asarray(pair[0]), np.asarray(pair[1])
        if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or (np.diff(ptr) < 0).any() or int(ptr[-1]) != len(ids):
            raise ValueError("a clause list is a CSR: ptr starts at 0, ascends and ends at the number of ids")
        if n_rows is not None and len(ptr) - 1 != n_rows:
            raise ValueError("the clause lists must agree on the row count")
        n_rows = len(ptr) - 1
        if len(ids) and (int(ids.min()) < -1 or int(ids.max()) >= rec.shape[0]):
            raise ValueError(f"clause ids must lie in [-1, {rec.shape[0]})")
    if n_rows is None:
        raise ValueError("give at least one of the all / any / none lists")


def check_collapse_args(columns, column, per_group, nulls) -> int:
    """What every collapse door checks of its keywords before anything is launched: ``column`` names a column of ``columns``
    (name -> :class:`HostColumn`) that can be a group key -- int32 / int64 / bool values or a category (collapsed by its code);
    a float32 and a set column are refused by name --, ``per_group`` >= 1 and ``nulls`` is "own", "one" or "drop".  Returns the
    SRX_COLLAPSE_NULL_* value.  Raises ValueError."""
    if column not in columns:
        raise ValueError(f"unknown field {column!r}")
    kind = columns[column].kind
    if kind in ("float32", "set"):
        raise ValueError(f"{column!r} is a {'float' if kind == 'float32' else 'set'} column: results collapse by an int32, int64 or category "
                         "column (float and set columns are no group keys)")
    if isinstance(per_group, bool) or not isinstance(per_group, (int, np.integer)) or not (1 <= int(per_group) <= I32_MAX):
        raise ValueError(f"per_group must be an integer in [1, {I32_MAX}], got {per_group!r}")
    if nulls not in NULL_POLICIES:
        raise ValueError(f"nulls must be one of {', '.join(NULL_POLICIES)}, got {nulls!r}")
    return NULL_POLICIES[nulls]


def check_order_args(columns, column, order, nulls):
    """What every ordering door checks of its keywords before anything is launched: ``column`` names a column of ``columns``
    (name -> :class:`HostColumn`) that has an order -- int32 / int64 / bool / float32 values or a category (ordered by its code,
    which is the string's place in the sorted dictionary); a set column is refused by name --, ``order`` is "asc" or "desc" and
    ``nulls`` is "last", "first" or "drop".  Returns ``(SRX_ORDER_*, SRX_ORDER_NULLS_*)``.  Raises ValueError."""
    if column not in columns:
        raise ValueError(f"unknown field {column!r}")
    if columns[column].kind == "set":
        raise ValueError(f"{column!r} is a set column: a label set has no order (order by a number or category column)")
    if not isinstance(order, str) or order not in ORDERS:
        raise ValueError(f"order must be one of {', '.join(ORDERS)}, got {order!r}")
    if not isinstance(nulls, str) or nulls not in ORDER_NULLS:
        raise ValueError(f"nulls must be one of {', '.join(ORDER_NULLS)}, got {nulls!r}")
    return ORDERS[order], ORDER_NULLS[nulls]


def decode_order_key(col: HostColumn, key: np.ndarray) -> np.ndarray:
    """``out_key`` words (int64) as values of the column's dtype: int32 narrowed, float32 from the bits in the low 32"""
    key = np.ascontiguousarray(key, dtype=np.int64)
    if col.type == _capi.SRX_FIELD_F32:
        return key.astype(np.uint32).view(np.float32)
    return key.astype(np.int32) if col.type == _capi.SRX_FIELD_I32 else key


class FacetSpec:
    """A binning spec resolved against one column (:func:`check_facet_args`): ``mode`` (SRX_FACET_*), ``n_bins``, ``origin`` (CODES),
    ``edges`` (EDGES: int64[n_bins + 1] as the device compares them -- exact bounds of the column's type, a float32's bits in the
    low 32 --, else None) and ``values`` = what bin i stands for in a result: a category string, a label, False / True, an int, or
    the ``(lo, hi)`` pair of the caller's own edges."""

    def __init__(self, mode: int, n_bins: int, origin: int = 0, edges: Optional[np.ndarray] = None, values=None):
        self.mode, self.n_bins, self.origin, self.edges, self.values = mode, n_bins, origin, edges, values


def _resolve_edges(column: str, kind: str, edges):
    """The caller's edges e_0 <= .. <= e_n as the int64 entries the device compares with, so that bin j holds exactly the column
    values >= e_j and < e_(j+1) in exact arithmetic: the smallest value of the column's type that is >= e_j."""
    if isinstance(edges, (str, bytes)) or not hasattr(edges, "__iter__"):
        raise ValueError(f"edges for {column!r} must be a sequence of at least two numbers")
    given = [_number(e, f"an edge for {column!r}") for e in edges]
    if len(given) < 2:
        raise ValueError(f"edges for {column!r} must be a sequence of at least two numbers (n + 1 edges make n bins)")
    if len(given) - 1 > _capi.SRX_FACET_MAX_BINS:
        raise ValueError(f"{len(given) - 1} bins for {column!r}: a facet takes at most {_capi.SRX_FACET_MAX_BINS}")
    if any(isinstance(e, float) and math.isnan(e) for e in given):
        raise ValueError(f"edges for {column!r} hold a NaN")
    if any(b < a for a, b in zip(given, given[1:])):
        raise ValueError(f"edges for {column!r} must ascend")
    out = np.zeros(len(given), dtype=np.int64)
    for j, e in enumerate(given):
        if kind == "float32":
            out[j] = f32_bits(f32_at_least(e))
        else:
            c = _int_ceil(e)
            if c > I64_MAX:
                if kind == "int64":
                    raise ValueError(f"the edge {e!r} for {column!r} lies above the int64 range: no int64 entry stands for it (leave the last bin to "
                                     f"end at {I64_MAX} and read the rest from \"other\")")
                c = I64_MAX  # above every int32 value either way
            out[j] = max(c, I64_MIN)
    return out, [(a, b) for a, b in zip(given, given[1:])]


def check_facet_args(columns, column, spec=None) -> FacetSpec:
    """What every facet door checks before anything is launched: ``column`` names a column of ``columns`` (name ->
    :class:`HostColumn`) and ``spec`` fits its kind.

      * category: no spec -- one bin per dictionary entry (SRX_FACET_CODES, origin 0); more than 8 192 entries raise ValueError;
      * bool: no spec -- the bins False and True;
      * set: no spec -- one bin per label (SRX_FACET_LABELS);
      * int32 / int64: ``{"origin": o, "bins": n}`` -- the bins o, o + 1, .., o + n - 1 (SRX_FACET_CODES) -- or ``{"edges": [...]}``;
      * float32: ``{"edges": [e_0, .., e_n]}`` -- bin j is [e_j, e_(j+1)) (SRX_FACET_EDGES), compared exactly: an edge that is no
        value of the column's type is rounded up to the next one (:func:`f32_at_least`, ``ceil``).

    ValueError: an unknown column, a spec that does not fit, edges that do not ascend or hold a NaN, more than 8 192 bins."""
    if column not in columns:
        raise ValueError(f"unknown field {column!r}")
    col = columns[column]
    kind = col.kind
    if kind in ("category", "bool", "set"):
        if spec is not None:
            raise ValueError(f"{column!r} is a {kind} column: its bins are its {'labels' if kind == 'set' else 'values'}, it takes no spec")
        if kind == "set":
            if not (1 <= len(col.dictionary) <= 64):
                raise ValueError(f"{column!r} has {len(col.dictionary)} labels: a set facet takes 1 to 64")
            return FacetSpec(_capi.SRX_FACET_LABELS, len(col.dictionary), values=list(col.dictionary))
        if kind == "bool":
            return FacetSpec(_capi.SRX_FACET_CODES, 2, 0, values=[False, True])
        if not (1 <= len(col.dictionary) <= _capi.SRX_FACET_MAX_BINS):
            raise ValueError(f"{column!r} has {len(col.dictionary)} distinct values: a facet takes at most {_capi.SRX_FACET_MAX_BINS} bins (a column "
                             "with more is a key to collapse by)")
        return FacetSpec(_capi.SRX_FACET_CODES, len(col.dictionary), 0, values=list(col.dictionary))
    if not isinstance(spec, dict) or not (set(spec) == {"edges"} or set(spec) == {"origin", "bins"}):
        raise ValueError(f"{column!r} is a {kind} column: give {{\"edges\": [...]}}" + ("" if kind == "float32" else " or {\"origin\": o, \"bins\": n}"))
    if "edges" in spec:
        edges, pairs = _resolve_edges(column, kind, spec["edges"])
        return FacetSpec(_capi.SRX_FACET_EDGES, len(pairs), edges=edges, values=pairs)
    if kind == "float32":
        raise ValueError(f"{column!r} is a float32 column: give {{\"edges\": [...]}} (a float is no bin number)")
    o, n = spec["origin"], spec["bins"]
    for x, what in ((o, "origin"), (n, "bins")):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise ValueError(f"{what} for {column!r} must be an integer, got {x!r}")
    o, n = int(o), int(n)
    if not (I64_MIN <= o <= I64_MAX):
        raise ValueError(f"origin for {column!r} lies outside int64")
    if not (1 <= n <= _capi.SRX_FACET_MAX_BINS):
        raise ValueError(f"{n} bins for {column!r}: a facet takes 1 to {_capi.SRX_FACET_MAX_BINS}")
    return FacetSpec(_capi.SRX_FACET_CODES, n, o, values=[o + i for i in range(n)])


class FieldTable:
    """Typed metadata columns of ``n_docs`` docs, resident on ``device``; row i of every column belongs to the doc with the GLOBAL
    id ``doc_base + i``.  ``columns`` name -> :class:`HostColumn` (kind, dictionary; its arrays are dropped after the upload)."""

    def __init__(self, columns: Dict[str, HostColumn], tensors, device, doc_base: int = 0):
        self.columns, self._tensors = columns, tensors
        self.device, self.doc_base = device, int(doc_base)
        self.n_docs = len(next(iter(columns.values())))

    @classmethod
    def from_columns(cls, columns, device="cuda:0", doc_base: int = 0) -> "FieldTable":
        """``columns``: name -> a sequence of n_docs entries (or an already prepared :class:`HostColumn`).  int32 / int64 /
        float32 arrays go up as they are (int8 / int16 / uint8 / uint16 widen to int32, uint32 to int64); ``bool`` becomes int32
        0 / 1; float64 raises ValueError (cast to float32: the device compares float32 values); a sequence of str / None becomes a
        CATEGORY column (int32 codes in the sorted order of the distinct strings, the dictionary stays here); a sequence of
        collections of str becomes a SET column (the labels as the bits of an int64; more than 64 distinct labels raise
        ValueError); None entries, and the masked entries of a ``numpy.ma`` array, become the column's validity row -- such a doc
        fails every test on the column."""
        torch = _torch()
        dev = torch.device(device)
        host = {str(n): (v if isinstance(v, HostColumn) else host_column(str(n), v)) for n, v in columns.items()} if isinstance(columns, dict) else None
        if not host:
            raise ValueError("columns must be a non-empty dict name -> sequence of n_docs entries")
        n_docs = len(next(iter(host.values())))
        if any(len(c) != n_docs for c in host.values()):
            raise ValueError("the columns must have one entry per doc each: their lengths differ")
        filter_words(n_docs)  # n_docs in [1, 2^31 - 2]
        tensors = {}
        for name, c in host.items():
            data = torch.from_numpy(c.data).to(dev)
            valid = None if c.valid is None else torch.from_numpy(pack_masks(c.valid).view(np.int32).copy()).to(dev).reshape(-1)
            tensors[name] = (data, valid)
        return cls(host, tensors, dev, doc_base)

    def device_bytes(self) -> int:
        """Bytes the columns and validity rows keep resident"""
        return sum(d.numel() * d.element_size() + (0 if v is None else v.numel() * 4) for d, v in self._tensors.values())

    def close(self) -> None:
        self._tensors = {}

    # -- the doors ------------------------------------------------------------------------------------------------------------
    def _col_descs(self, names):
        if not (1 <= len(names) <= _capi.SRX_FIELDS_MAX_COLS):
            raise ValueError(f"one call takes 1 to {_capi.SRX_FIELDS_MAX_COLS} columns, got {len(names)}")
        arr = (_capi.FieldColDesc * len(names))()
        for i, name in enumerate(names):
            if name not in self._tensors:
                raise ValueError(f"unknown field {name!r}" if name not in self.columns else "the table is closed")
            data, valid = self._tensors[name]
            arr[i].data, arr[i].valid, arr[i].type = data.data_ptr(), (None if valid is None else valid.data_ptr()), self.columns[name].type
        return arr

    def _col_desc(self, column: str):
        """The descriptor of one named column; ValueError "unknown field" / "the table is closed" """
        return self._col_descs([column])

    def _list_triple(self, who: str, cap, doc, score, count, scored: bool = True):
        """The ``(doc, score, count)`` device tensors of result lists, checked for the door ``who``: doc int32 [nq, m], m in
        [1, cap] (``cap`` None: m >= 1), score float32 of doc's shape (not looked at unless ``scored``), count int32 [nq] or None,
        all on the table's device.  Returns them contiguous, then nq and m."""
        torch = _torch()
        if not isinstance(doc, torch.Tensor) or doc.dim() != 2 or doc.dtype != torch.int32 or (cap is None and int(doc.shape[1]) < 1):
            raise ValueError(f"{who}: doc must be an int32 tensor [nq, m{'' if cap else ' >= 1'}]")
        nq, m = int(doc.shape[0]), int(doc.shape[1])
        if cap is not None and not (1 <= m <= cap):
            raise ValueError(f"{who} takes lists of 1 to {cap} positions, got {m} (no silent truncation)")
        if not scored:
            score = None
        elif not isinstance(score, torch.Tensor) or score.dtype != torch.float32 or tuple(score.shape) != (nq, m):
            raise ValueError(f"{who}: score must be a float32 tensor of doc's shape")
        if count is not None and (not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.numel() != nq):
            raise ValueError(f"{who}: count must be an int32 tensor [nq]")
        for t, what in ((doc, "doc"), (score, "score"), (count, "count")):
            if t is not None and t.device != self.device:
                raise ValueError(f"{who}: {what} is on {t.device}, the table on {self.device}")
        return doc.contiguous(), None if score is None else score.contiguous(), None if count is None else count.contiguous(), nq, m

    @staticmethod
    def _check_k(who: str, k, top: int, top_name: str = "m") -> int:
        k = int(k)
        if not (1 <= k <= top):
            raise ValueError(f"{who}: k must be in [1, {top_name} = {top}], got {k}")
        return k

    def _filter_rows(self, filter, q_filter, n_rows):
        """The ``filter`` / ``q_filter`` / ``n_rows`` keywords of a door over filter rows (:meth:`facet_device`) resolved: the
        number of output rows and the device ``q_filter`` of the launch -- 0, 1, .. when output row r is filter row r."""
        torch = _torch()
        if filter is None:
            if q_filter is not None:
                raise ValueError("q_filter picks rows of a filter: it needs filter=")
            n_rows = 1 if n_rows is None else int(n_rows)
        else:
            if not isinstance(filter, DocFilter):
                raise ValueError("filter must be a DocFilter")
            filter.for_index(self)
            if n_rows is None:
                n_rows = filter.n_filters if q_filter is None else int(q_filter.numel())
            n_rows = int(n_rows)
            if q_filter is None and (n_rows > 1 or filter.n_filters > 1):  # row r of the output is row r of the filter
                if n_rows > filter.n_filters:
                    raise ValueError(f"n_rows = {n_rows} exceeds the filter's {filter.n_filters} rows: give q_filter")
                q_filter = torch.arange(n_rows, dtype=torch.int32, device=self.device)
        if n_rows < 0:
            raise ValueError("n_rows must be >= 0")
        return n_rows, q_filter

    @staticmethod
    def _host_q_filter(filter, q_filter):
        """A host ``q_filter`` sequence validated (integers in [-1, n_filters)) and uploaded; None stays None"""
        if q_filter is None:
            return None
        if not isinstance(filter, DocFilter):
            raise ValueError("q_filter picks rows of a filter: it needs filter=")
        q = np.asarray(q_filter)
        return q_filter_to_device(filter, q, int(q.shape[0]) if q.ndim == 1 else -1)

    def _host_lists(self, who: str, cap, doc, score, count, scored: bool = True, score_name: str = "score"):
        """Host result lists for the door ``who``: validated (:func:`~.index.validate_candidates`), at most ``cap`` positions deep
        (None: any depth), the score of doc's shape (unless not ``scored``); uploaded as ``(doc, score | None, count | None)``."""
        from .index import validate_candidates
        torch = _torch()
        d = np.asarray(doc)
        d, c = validate_candidates(d, count, int(d.shape[0]) if d.ndim == 2 else 0)
        if cap is not None and d.shape[1] > cap:
            raise ValueError(f"{who} takes lists of at most {cap} positions, got {d.shape[1]} (no silent truncation)")
        s = None
        if scored:
            s = np.ascontiguousarray(score, dtype=np.float32)
            if s.shape != d.shape:
                raise ValueError(f"{score_name} must have doc's shape")
            s = torch.as_tensor(s, device=self.device)
        return torch.as_tensor(d, device=self.device), s, None if c is None else torch.as_tensor(c, device=self.device)

    def _to_host(self, tensors):
        """One synchronisation, then every tensor as a NumPy array"""
        _torch().cuda.synchronize(self.device)
        return tuple(t.cpu().numpy() for t in tensors)

    def filter_device(self, clauses, values=None, all=None, any=None, none=None, columns=None, base=None, q_base=None, out=None) -> DocFilter:
        """``srx_filter_from_fields`` on device tensors.  ``clauses``: int64 [n_clauses, 3], one (col | op << 32, lo, hi) record
        per row (the 24 bytes of ``srx_field_clause``); ``values``: int64 [n_values] or None; each of ``all`` / ``any`` /
        ``none``: None or a ``(ptr, clause)`` pair of int32 tensors, a CSR over the output rows (at least one is given, and they
        agree on the row count); ``columns``: the names a record's ``col`` indexes (default: every column of the table, in
        order; at most 32).  ``base`` / ``q_base`` / ``out`` as in :meth:`~.index.DeviceIndex.term_filter_device`.  Returns a
        DocFilter over the table's ``n_docs`` / ``doc_base``; asynchronous on the current stream.  Precondition (NOT checked
        here, the tensors never leave the device): what :func:`check_records` checks of host arrays, and q_base in
        [-1, n_filters)."""
        torch = _torch()
        names = list(self.columns) if columns is None else list(columns)
        descs = self._col_descs(names)

        def check(t, dtype, what, dim=1):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or t.dim() != dim:
                raise ValueError(f"{what} must be a {dim}-D {dtype} tensor on {self.device}")
            return t.contiguous()

        clauses = check(clauses, torch.int64, "clauses", 2)
        if clauses.shape[1] != 3:
            raise ValueError("clauses must be int64 [n_clauses, 3]")
        if values is not None:
            values = check(values, torch.int64, "values")

        def launch(n_rows, lists, bdesc, out_ptr, stream):
            return _capi.lib().srx_filter_from_fields(self.device.index or 0, self.n_docs, descs, len(names), _ptr(clauses), int(clauses.shape[0]),
                                                      _ptr(values), n_rows, *lists, bdesc, out_ptr, stream)
        return build_rows(self, "srx_filter_from_fields", launch, (all, any, none), "clause", base, q_base, out)

    def filter_arrays(self, clauses, values, all=None, any=None, none=None, columns=None, base=None, q_base=None) -> DocFilter:
        """:meth:`filter_device` from host arrays, validated first (:func:`check_records`: cols, ops against the column types, IN
        ranges, clause ids; ``q_base`` with :func:`~.filter.validate_q_filter`)."""
        torch = _torch()
        names = list(self.columns) if columns is None else list(columns)
        for name in names:
            if name not in self.columns:
                raise ValueError(f"unknown field {name!r}")
        values = np.zeros(0, np.int64) if values is None else np.ascontiguousarray(values, dtype=np.int64)
        clauses = np.ascontiguousarray(clauses, dtype=np.int64).reshape(-1, 3)
        check_records([self.columns[n].type for n in names], clauses, len(values), (all, any, none))
        n_rows = next(len(p[0]) - 1 for p in (all, any, none) if p is not None)
        qb = host_q_filter(self, base, q_base, n_rows, BASE_NAMES)
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.device)
        pairs = [None if p is None else (up(p[0], np.int32), up(p[1], np.int32)) for p in (all, any, none)]
        return self.filter_device(up(clauses, np.int64), up(values, np.int64) if len(values) else None, *pairs, columns=names, base=base, q_base=qb)

    def filter(self, where, base=None, q_base=None) -> DocFilter:
        """Filter rows from a predicate.  ``where``: one group, or a list of groups -- one per output row.  A group is
        ``{"must": [...], "should": [...], "must_not": [...]}`` (any of the three absent): a doc passes when EVERY ``must`` clause
        holds, at least one ``should`` clause (when there are any) and NO ``must_not`` clause; a bare list of clauses is ``must``.
        A clause is a dict with ``"field"`` and one test:

          * ``gte`` / ``gt`` / ``lte`` / ``lt``  (combinable) on number columns -- compared exactly: a bound that is not a value
            of the column's type is rounded towards the inside of the range, so ``{"gte": 0.1}`` on a float32 column admits
            exactly the float32 values >= 0.1;
          * ``eq``  and ``in``  on number and category columns (a value no entry can equal, an unknown category: no doc);
          * ``any_of`` / ``all_of``  on set columns: the doc carries one / every listed label (``all_of`` with an unknown label: no doc);
          * ``exists: True``  the doc has a value.  On a float32 column this is the full range, so a NaN counts as missing.

        A doc WITHOUT a value fails every test, so it passes a clause under ``must_not``.  ``base`` / ``q_base``: a
        :class:`~.filter.DocFilter` over the same docs the rows are intersected with, and the base row of every output row (a host
        sequence; None: row 0; -1: none).  A table of more than 32 columns passes the ones the clauses name; a call that names
        more raises ValueError.  Memory: n_rows * n_docs / 8 bytes."""
        res = WhereResolver(self.columns)
        for g in where_groups(where):
            res.add(g)
        return self.filter_resolved(res, base=base, q_base=q_base)

    def filter_resolved(self, res: WhereResolver, rows=None, base=None, q_base=None) -> DocFilter:
        """The rows of a :class:`WhereResolver` over this table's columns (``rows``: other triples of its clause ids)"""
        rec, values, lists = res.arrays(rows)
        names = res.names or list(self.columns)[:1]  # no clause: any column serves
        if len(names) > _capi.SRX_FIELDS_MAX_COLS:
            raise ValueError(f"the predicate names {len(names)} fields: one call takes at most {_capi.SRX_FIELDS_MAX_COLS}")
        return self.filter_arrays(rec, values, *lists, columns=names, base=base, q_base=q_base)

    # -- collapsing ranked lists by a column (include/sparse_rx_collapse.h) ---------------------------------------------------
    def collapse_device(self, column: str, doc, score, count, k: int, per_group: int = 1, nulls: str = "own", want_pos: bool = False,
                        want_group_size: bool = False):
        """``srx_collapse_topk`` on device tensors: the first ``k`` positions of every list that have fewer than ``per_group``
        earlier positions of their group, the group being the value ``column`` holds for the doc (a category column collapses
        by its code).  ``doc`` i32[nq, m] GLOBAL ids, ``score`` f32[nq, m], ``count`` i32[nq] or None: the triple of any search,
        of the fusion or of a reranker as it is, m <= 2048, 1 <= k <= m.  A position at or past the count, or with an id outside
        the table, is skipped; scores are copied, never looked at.  ``nulls``: a doc without a value is a group of its "own"
        (it always survives), all of them are "one" group, or they "drop" out.  Returns device tensors ``(doc i32[nq, k], score
        f32[nq, k], count i32[nq])`` -- a subsequence of each list, rows padded with -1 / 0 --, then ``pos`` i32[nq, k] (the
        survivor's position in the list given) with ``want_pos`` and ``group_size`` i32[nq, k] (the live positions OF THE LIST
        GIVEN in its group) with ``want_group_size``.  Asynchronous on the current stream, one launch.  ValueError: an unknown
        column, a float or set column, m > 2048, k outside [1, m], tensors of another dtype, shape or device."""
        torch = _torch()
        policy = check_collapse_args(self.columns, column, per_group, nulls)
        desc = self._col_desc(column)
        doc, score, count, nq, m = self._list_triple("collapse_device", _capi.SRX_COLLAPSE_MAX_M, doc, score, count)
        k = self._check_k("collapse_device", k, m)
        with torch.cuda.device(self.device):
            outs = [torch.empty((nq, k), dtype=torch.int32, device=self.device), torch.empty((nq, k), dtype=torch.float32, device=self.device),
                    torch.empty((nq,), dtype=torch.int32, device=self.device)]
            pos = torch.empty((nq, k), dtype=torch.int32, device=self.device) if want_pos else None
            size = torch.empty((nq, k), dtype=torch.int32, device=self.device) if want_group_size else None
            rc = _capi.lib().srx_collapse_topk(self.device.index or 0, desc, self.n_docs, self.doc_base, _ptr(doc), _ptr(score), _ptr(count), nq, m, k,
                                               int(per_group), policy, *[_ptr(o) for o in outs], _ptr(pos), _ptr(size),
                                               torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(rc, "srx_collapse_topk")
        return tuple(outs + [t for t in (pos, size) if t is not None])

    def collapse(self, column: str, doc, score, count, k: int, per_group: int = 1, nulls: str = "own", want_pos: bool = False,
                 want_group_size: bool = False):
        """Host arrays in (the candidates validated by :func:`~.index.validate_candidates`), host arrays out:
        :meth:`collapse_device` with one synchronisation and one copy back."""
        check_collapse_args(self.columns, column, per_group, nulls)
        lists = self._host_lists("collapse", _capi.SRX_COLLAPSE_MAX_M, doc, score, count)
        return self._to_host(self.collapse_device(column, *lists, k, per_group, nulls, want_pos, want_group_size))

    # -- facet counts over filter rows and result lists (include/sparse_rx_facets.h) -------------------------------------------
    def _facet_call(self, column: str, spec):
        """(the resolved :class:`FacetSpec`, the column descriptor, the ``srx_facet_bins`` struct, what must stay alive)"""
        torch = _torch()
        fs = spec if isinstance(spec, FacetSpec) else check_facet_args(self.columns, column, spec)
        desc = self._col_desc(column)
        edges = None if fs.edges is None else torch.as_tensor(fs.edges, device=self.device)
        bins = _capi.FacetBins(mode=fs.mode, n_bins=fs.n_bins, origin=fs.origin, edges=None if edges is None else edges.data_ptr())
        return fs, desc, bins, edges

    def facet_device(self, column: str, spec=None, filter=None, q_filter=None, n_rows=None):
        """``srx_facet_counts``: how the docs of filter rows distribute over ``column``.  ``spec`` as :func:`check_facet_args` takes
        it (or its result); ``filter``: a :class:`~.filter.DocFilter` over this table's docs, or None = every doc; ``q_filter``: an
        int32 device tensor [n_rows], the filter row of every output row (-1: every doc), or None.  ``n_rows`` defaults to the
        filter's row count with ``q_filter`` = 0, 1, .. when neither is given, to ``q_filter``'s length when it is, and to 1 without
        a filter.  Returns device tensors ``(counts i32[n_rows, n_bins], extra i32[n_rows, 3])``, extra = (missing, other, total)
        per row; asynchronous on the current stream."""
        import ctypes
        torch = _torch()
        fs, desc, bins, edges = self._facet_call(column, spec)
        n_rows, q_filter = self._filter_rows(filter, q_filter, n_rows)
        fdesc, keep = (None, None) if filter is None else filter.launch_args(q_filter, n_rows)
        with torch.cuda.device(self.device):
            counts = torch.empty((n_rows, fs.n_bins), dtype=torch.int32, device=self.device)
            extra = torch.empty((n_rows, 3), dtype=torch.int32, device=self.device)
            rc = _capi.lib().srx_facet_counts(self.device.index or 0, desc, self.n_docs, ctypes.byref(bins), fdesc, n_rows,
                                              counts.data_ptr() if n_rows else None, extra.data_ptr() if n_rows else None,
                                              torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(rc, "srx_facet_counts")
        del keep, edges
        return counts, extra

    def facet_lists_device(self, column: str, doc, count, spec=None):
        """``srx_facet_counts_lists``: how the docs of result lists distribute over ``column``.  ``doc`` i32[nq, m] GLOBAL ids and
        ``count`` i32[nq] or None: the lists of any search as they are (a position at or past the count, or with an id outside the
        table, is skipped; a doc listed twice counts twice).  Returns ``(counts i32[nq, n_bins], extra i32[nq, 3])`` on the device;
        asynchronous on the current stream."""
        import ctypes
        torch = _torch()
        fs, desc, bins, edges = self._facet_call(column, spec)
        doc, _, count, nq, m = self._list_triple("facet_lists_device", None, doc, None, count, scored=False)
        with torch.cuda.device(self.device):
            counts = torch.empty((nq, fs.n_bins), dtype=torch.int32, device=self.device)
            extra = torch.empty((nq, 3), dtype=torch.int32, device=self.device)
            rc = _capi.lib().srx_facet_counts_lists(self.device.index or 0, desc, self.n_docs, self.doc_base, ctypes.byref(bins), _ptr(doc), _ptr(count),
                                                    nq, m, _ptr(counts), _ptr(extra), torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(rc, "srx_facet_counts_lists")
        del edges
        return counts, extra

    def facet(self, column: str, spec=None, filter=None, q_filter=None, n_rows=None):
        """:meth:`facet_device` with a host ``q_filter`` (validated: integers in [-1, n_filters)) and host arrays back: one
        synchronisation, one copy."""
        return self._counts_to_host(*self.facet_device(column, spec, filter, self._host_q_filter(filter, q_filter), n_rows))

    def facet_lists(self, column: str, doc, count=None, spec=None):
        """:meth:`facet_lists_device` from host arrays (the candidates validated by :func:`~.index.validate_candidates`), host arrays
        back: one synchronisation, one copy."""
        fs = spec if isinstance(spec, FacetSpec) else check_facet_args(self.columns, column, spec)
        d, _, c = self._host_lists("facet_lists", None, doc, None, count, scored=False)
        return self._counts_to_host(*self.facet_lists_device(column, d, c, fs))

    @staticmethod
    def _counts_to_host(counts, extra):
        """``(counts, extra)`` of a facet door as host arrays: one copy, which synchronises"""
        both = _torch().cat([counts, extra], dim=1).cpu().numpy()
        return both[:, : counts.shape[1]], both[:, counts.shape[1]:]

    # -- ordering filter rows and result lists by a column (include/order/sparse_rx_order.h) ------------------------------------
    def top_by_device(self, column: str, k: int, order: str = "desc", nulls: str = "last", filter=None, q_filter=None, n_rows=None, after=None):
        """``srx_order_topk``: the first ``k`` docs (1 <= k <= 1024) of filter rows in the order of ``column`` -- "asc" or "desc",
        equal values by ascending doc id; docs without a value (a float NaN is one) ``nulls`` = "last", "first", or "drop"ped.
        ``filter`` / ``q_filter`` / ``n_rows`` as :meth:`facet_device` takes them.  ``after``: an int32 device tensor [n_rows] of
        GLOBAL doc ids, the cursor of every row (-1: none; the last doc of the previous page continues it), or None.  Returns
        device tensors ``(doc i32[n_rows, k], key i64[n_rows, k], extra i32[n_rows, 3])``, extra = (count, valued, total) per
        row, rows padded with -1 / 0; asynchronous on the current stream, no synchronisation."""
        torch = _torch()
        o, nl = check_order_args(self.columns, column, order, nulls)
        desc = self._col_desc(column)
        k = int(k)
        if not (1 <= k <= _capi.SRX_MAX_K):
            raise ValueError(f"top_by_device: k must be in [1, {_capi.SRX_MAX_K}], got {k} (page with after=)")
        n_rows, q_filter = self._filter_rows(filter, q_filter, n_rows)
        if after is not None and (not isinstance(after, torch.Tensor) or after.dtype != torch.int32 or after.numel() != n_rows or after.device != self.device):
            raise ValueError(f"top_by_device: after must be an int32 tensor [n_rows] on {self.device}")
        fdesc, keep = (None, None) if filter is None else filter.launch_args(q_filter, n_rows)
        _, ws_bytes = _capi.order_plan(self.n_docs, n_rows, k)
        with torch.cuda.device(self.device):
            after = None if after is None else after.contiguous()
            doc = torch.empty((n_rows, k), dtype=torch.int32, device=self.device)
            key = torch.empty((n_rows, k), dtype=torch.int64, device=self.device)
            extra = torch.empty((n_rows, 3), dtype=torch.int32, device=self.device)
            ws = torch.empty(((ws_bytes + 15) // 8,), dtype=torch.int64, device=self.device)
            rc = _capi.lib().srx_order_topk(self.device.index or 0, desc, self.n_docs, self.doc_base, o, nl, fdesc, n_rows, k, _ptr(after), _ptr(doc),
                                            _ptr(key), _ptr(extra), ws.data_ptr(), ws.numel() * 8, torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(rc, "srx_order_topk")
        del keep
        return doc, key, extra

    def top_by(self, column: str, k: int, order: str = "desc", nulls: str = "last", filter=None, q_filter=None, n_rows=None, after=None):
        """:meth:`top_by_device` with host ``q_filter`` / ``after`` sequences (validated) and host arrays back: ``(doc i32[n_rows, k],
        key [n_rows, k] in the column's dtype, has_value bool[n_rows, k], extra i32[n_rows, 3])``.  One synchronisation."""
        torch = _torch()
        check_order_args(self.columns, column, order, nulls)
        qf = self._host_q_filter(filter, q_filter)
        af = None
        if after is not None:
            a = np.asarray(after)
            if a.ndim != 1 or a.dtype.kind not in "iu" or (len(a) and (int(a.min()) < I32_MIN or int(a.max()) > I32_MAX)):
                raise ValueError("after must be a 1-D sequence of int32 doc ids (-1: no cursor)")
            af = torch.as_tensor(a.astype(np.int32), device=self.device)
        doc, key, extra = self._to_host(self.top_by_device(column, k, order, nulls, filter, qf, n_rows, af))
        return doc, decode_order_key(self.columns[column], key), order_has_value(extra, nulls, doc.shape[1]), extra

    def sort_lists_device(self, column: str, doc, score, count, k: int, order: str = "desc", nulls: str = "last", want_pos: bool = False):
        """``srx_order_lists`` on device tensors: the first ``k`` live positions of every list, STABLY sorted by the value
        ``column`` holds for the doc (equal values and valueless docs keep their list order).  ``doc`` i32[nq, m] GLOBAL ids,
        ``score`` f32[nq, m], ``count`` i32[nq] or None, as :meth:`collapse_device` takes them; m <= 2048, 1 <= k <= m.  Returns
        device tensors ``(doc i32[nq, k], score f32[nq, k], key i64[nq, k], extra i32[nq, 3])``, extra = (count, valued, live),
        then ``pos`` i32[nq, k] with ``want_pos``; rows padded with -1 / 0 / 0 / -1.  Asynchronous on the current stream, one launch."""
        torch = _torch()
        o, nl = check_order_args(self.columns, column, order, nulls)
        desc = self._col_desc(column)
        doc, score, count, nq, m = self._list_triple("sort_lists_device", _capi.SRX_ORDER_MAX_M, doc, score, count)
        k = self._check_k("sort_lists_device", k, m)
        with torch.cuda.device(self.device):
            outs = [torch.empty((nq, k), dtype=torch.int32, device=self.device), torch.empty((nq, k), dtype=torch.float32, device=self.device),
                    torch.empty((nq, k), dtype=torch.int64, device=self.device)]
            pos = torch.empty((nq, k), dtype=torch.int32, device=self.device) if want_pos else None
            extra = torch.empty((nq, 3), dtype=torch.int32, device=self.device)
            rc = _capi.lib().srx_order_lists(self.device.index or 0, desc, self.n_docs, self.doc_base, o, nl, _ptr(doc), _ptr(score), _ptr(count), nq, m, k,
                                             *[_ptr(t) for t in outs], _ptr(pos), _ptr(extra), torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(rc, "srx_order_lists")
        return tuple(outs + [extra] + ([pos] if want_pos else []))

    def sort_lists(self, column: str, doc, score, count, k: int, order: str = "desc", nulls: str = "last", want_pos: bool = False):
        """Host arrays in (the candidates validated by :func:`~.index.validate_candidates`), host arrays out:
        :meth:`sort_lists_device` with one synchronisation and one copy back; ``key`` stays int64 (:func:`decode_order_key`)."""
        check_order_args(self.columns, column, order, nulls)
        lists = self._host_lists("sort_lists", _capi.SRX_ORDER_MAX_M, doc, score, count)
        return self._to_host(self.sort_lists_device(column, *lists, k, order, nulls, want_pos))

    # -- boosting ranked lists by column values (include/boost/sparse_rx_boost.h) ----------------------------------------------
    def boost_device(self, columns, clauses, knots, score_mode: int, boost_mode: int, doc, score, count, k: int, carry=None,
                     want_pos: bool = False):
        """``srx_boost_topk`` on device tensors: the raw scores of every list moved by the clauses' curves over ``columns`` (the
        names a clause's ``col`` indexes, 1 to 8, none a set column), and the first ``k`` by (new score descending, doc id
        ascending).  ``clauses``: a uint8 tensor [n_clauses, 40], the records of ``srx_boost_clause`` (``boost.CLAUSE_DTYPE``);
        ``knots``: float32 [n_knots]; ``score_mode`` / ``boost_mode``: SRX_BOOST_*.  ``doc`` i32[nq, m] GLOBAL ids, ``score``
        f32[nq, m] RAW scores in any order, ``count`` i32[nq] or None.  ``carry``: None or ``(doc i32[nq, kc], score f32[nq, kc],
        count i32[nq] | None)`` whose scores are FINAL; m + kc <= 2048, 1 <= k <= m + kc.  Returns device tensors ``(doc i32[nq, k],
        score f32[nq, k], count i32[nq])`` padded with -1 / 0, then ``pos`` i32[nq, k] (the position in carry ++ candidates)
        with ``want_pos``.  Asynchronous on the current stream, one launch.  Precondition (NOT checked here, the tensors never
        leave the device): what :func:`~.boost.check_clause_arrays` checks of host arrays."""
        torch = _torch()
        names = [columns] if isinstance(columns, str) else list(columns)
        if not (1 <= len(names) <= _capi.SRX_BOOST_MAX_COLS):
            raise ValueError(f"a boost takes 1 to {_capi.SRX_BOOST_MAX_COLS} columns, got {len(names)}")
        for name in names:
            if name not in self.columns:
                raise ValueError(f"unknown field {name!r}")
            if self.columns[name].kind == "set":
                raise ValueError(f"{name!r} is a set column: a label set is no number to boost by")
        descs = self._col_descs(names)

        def check(t, dtype, what, shape=None, dim=None):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or (shape is not None and tuple(t.shape) != shape) or (dim is not None and t.dim() != dim):
                raise ValueError(f"boost_device: {what} must be a {dtype} tensor" + (f" of shape {shape}" if shape is not None else f" with {dim} dims"))
            if t.device != self.device:
                raise ValueError(f"boost_device: {what} is on {t.device}, the table on {self.device}")
            return t.contiguous()

        clauses = check(clauses, torch.uint8, "clauses", dim=2)
        if clauses.shape[1] != 40 or not (1 <= int(clauses.shape[0]) <= _capi.SRX_BOOST_MAX_CLAUSES):
            raise ValueError(f"boost_device: clauses must be uint8 [1 .. {_capi.SRX_BOOST_MAX_CLAUSES}, 40]")
        knots = check(knots, torch.float32, "knots", dim=1)
        if not (2 <= knots.numel() <= _capi.SRX_BOOST_MAX_KNOTS):
            raise ValueError("boost_device: knots must hold 2 to 2^24 entries")
        doc = check(doc, torch.int32, "doc", dim=2)
        nq, m = int(doc.shape[0]), int(doc.shape[1])
        score = check(score, torch.float32, "score", shape=(nq, m))
        if count is not None:
            count = check(count.reshape(-1) if isinstance(count, torch.Tensor) else count, torch.int32, "count", shape=(nq,))
        cd = cs = cc = None
        kc = 0
        if carry is not None:
            cd = check(carry[0], torch.int32, "carry doc", dim=2)
            kc = int(cd.shape[1])
            if int(cd.shape[0]) != nq or kc < 1:
                raise ValueError("boost_device: carry doc must be int32 [nq, kc >= 1]")
            cs = check(carry[1], torch.float32, "carry score", shape=(nq, kc))
            if len(carry) > 2 and carry[2] is not None:
                cc = check(carry[2].reshape(-1) if isinstance(carry[2], torch.Tensor) else carry[2], torch.int32, "carry count", shape=(nq,))
        if m < 1 or m + kc > _capi.SRX_BOOST_MAX_M:
            raise ValueError(f"boost_device takes lists of 1 to {_capi.SRX_BOOST_MAX_M} positions, carry included, got {m} + {kc} (no silent truncation)")
        k = self._check_k("boost_device", k, m + kc, "m + kc")
        with torch.cuda.device(self.device):
            outs = [torch.empty((nq, k), dtype=torch.int32, device=self.device), torch.empty((nq, k), dtype=torch.float32, device=self.device),
                    torch.empty((nq,), dtype=torch.int32, device=self.device)]
            pos = torch.empty((nq, k), dtype=torch.int32, device=self.device) if want_pos else None
            rc = _capi.lib().srx_boost_topk(self.device.index or 0, descs, len(names), self.n_docs, self.doc_base, _ptr(clauses), int(clauses.shape[0]),
                                            _ptr(knots), int(knots.numel()), int(score_mode), int(boost_mode), _ptr(doc), _ptr(score), _ptr(count),
                                            _ptr(cd), _ptr(cs), _ptr(cc), nq, m, kc, k, *[_ptr(o) for o in outs], _ptr(pos),
                                            torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(rc, "srx_boost_topk")
        return tuple(outs + ([pos] if want_pos else []))

    def boost(self, boost, doc, score, count, k: int, carry=None, want_pos: bool = False):
        """Host arrays in, host arrays out: ``boost`` is a spec :class:`~.boost.BoostResolver` takes (or a resolver over this
        table's columns), the candidates (and the carry's) are validated by :func:`~.index.validate_candidates`, the clause
        records by :func:`~.boost.check_clause_arrays`; then :meth:`boost_device` with one synchronisation and one copy back."""
        from .boost import BoostFn, BoostResolver, check_clause_arrays
        res = boost if isinstance(boost, BoostResolver) else BoostResolver(self.columns, boost)
        check_clause_arrays([self.columns[n].type for n in res.names], res.clauses, res.knots)
        cand = self._host_lists("boost", None, doc, score, count, score_name="the score")  # the depth cap counts the carry in: below
        kc = 0 if carry is None else int(np.asarray(carry[0]).shape[1])
        if int(cand[0].shape[1]) + kc > _capi.SRX_BOOST_MAX_M:
            raise ValueError(f"boost takes lists of at most {_capi.SRX_BOOST_MAX_M} positions, carry included (no silent truncation)")
        cr = None if carry is None else self._host_lists("boost", None, carry[0], carry[1], carry[2] if len(carry) > 2 else None,
                                                         score_name="the carry's score")
        return self._to_host(BoostFn(self, res)(*cand, k, carry=cr, want_pos=want_pos))

    # -- reranking ranked lists with a tree-ensemble model (include/ltr/sparse_rx_ltr.h) ----------------------------------------
    @classmethod
    def without_columns(cls, n_docs: int, device="cuda:0", doc_base: int = 0) -> "FieldTable":
        """A table of ``n_docs`` docs that holds no column: what :meth:`rank_model_device` needs when no feature names one"""
        filter_words(int(n_docs))  # n_docs in [1, 2^31 - 2]
        table = cls.__new__(cls)
        table.columns, table._tensors = {}, {}
        table.device, table.doc_base, table.n_docs = _torch().device(device), int(doc_base), int(n_docs)
        return table

    def _rank_call(self, who: str, model, features, doc, score, count, extra, mode, named_extra):
        """What the two model doors share: the features resolved against this table's columns, the column descriptors, the lists
        through the one list door, the extra plane checked -> the leading arguments of ``srx_ltr_topk`` / ``srx_ltr_score`` up to
        ``m``, and what must stay alive until the launch."""
        from .ltr import ForestModel, check_mode, feature_array, resolve_features, CMPS
        torch = _torch()
        if not isinstance(model, ForestModel):
            raise ValueError(f"{who}: model must be a ForestModel (ForestModel.from_arrays / from_sklearn)")
        mode_id = check_mode(mode)
        records, names, n_extra = resolve_features(self.columns, features, model, named_extra)
        descs = self._col_descs(names) if names else None
        doc, score, count, nq, m = self._list_triple(who, _capi.SRX_LTR_MAX_M, doc, score, count)
        if n_extra == 0:
            extra = None  # not looked at
        else:
            if not isinstance(extra, torch.Tensor) or extra.dtype != torch.float32 or extra.dim() != 3 or tuple(extra.shape[:2]) != (nq, m):
                raise ValueError(f"{who}: the features name extra values: extra must be a float32 tensor [nq, m, n_extra]")
            if not (n_extra <= int(extra.shape[2]) <= _capi.SRX_LTR_MAX_EXTRA):
                raise ValueError(f"{who}: extra holds {int(extra.shape[2])} values per position, the features need {n_extra} (at most {_capi.SRX_LTR_MAX_EXTRA})")
            if extra.device != self.device:
                raise ValueError(f"{who}: extra is on {extra.device}, the table on {self.device}")
            extra = extra.contiguous()
        nodes, tree_ptr = model.to_device(self.device)
        feats = feature_array(records)
        head = (self.device.index or 0, descs, len(names), self.n_docs, self.doc_base, feats, len(records), _ptr(extra),
                0 if extra is None else int(extra.shape[2]), nodes.data_ptr(), model.n_nodes, tree_ptr.data_ptr(), model.n_trees,
                float(model.base), CMPS[model.cmp], mode_id, _ptr(doc), _ptr(score), _ptr(count), nq, m)
        return head, nq, m, (descs, feats, extra, nodes, tree_ptr, doc, score, count)

    def rank_model_device(self, model, features, doc, score, count, k: int, extra=None, mode: str = "replace", want_pos: bool = False,
                          named_extra=()):
        """``srx_ltr_topk`` on device tensors: the score of every live position of every list replaced by (``mode`` "replace") or
        moved by (``mode`` "sum": raw score + model) the output of ``model`` (a :class:`~.ltr.ForestModel`) over ``features`` --
        a list whose entry f is the model's feature f: "score" (the raw score), "rank" (the position), the name of a number column
        of this table (a doc without a value, or a float NaN, is MISSING), or ``("extra", i)`` = ``extra[q, c, i]`` of the float32
        device tensor ``extra`` [nq, m, n_extra <= 32] (a NaN is missing) -- and the first ``k`` by (new score descending, doc id
        ascending).  ``doc`` i32[nq, m] GLOBAL ids, ``score`` f32[nq, m], ``count`` i32[nq] or None, m <= 2048, 1 <= k <= m.
        Returns device tensors ``(doc i32[nq, k], score f32[nq, k], count i32[nq])`` padded with -1 / 0, then ``pos`` i32[nq, k]
        (the position in the list given) with ``want_pos``.  Asynchronous on the current stream, one launch.  ``named_extra``:
        names that stand for the first extra slots (:func:`~.ltr.resolve_features`)."""
        torch = _torch()
        head, nq, m, keep = self._rank_call("rank_model_device", model, features, doc, score, count, extra, mode, named_extra)
        k = self._check_k("rank_model_device", k, m)
        with torch.cuda.device(self.device):
            outs = [torch.empty((nq, k), dtype=torch.int32, device=self.device), torch.empty((nq, k), dtype=torch.float32, device=self.device),
                    torch.empty((nq,), dtype=torch.int32, device=self.device)]
            pos = torch.empty((nq, k), dtype=torch.int32, device=self.device) if want_pos else None
            rc = _capi.lib().srx_ltr_topk(*head, k, *[_ptr(o) for o in outs], _ptr(pos), torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(rc, "srx_ltr_topk")
        del keep
        return tuple(outs + ([pos] if want_pos else []))

    def model_scores_device(self, model, features, doc, score, count, extra=None, mode: str = "replace", named_extra=()):
        """``srx_ltr_score`` on device tensors: the inputs of :meth:`rank_model_device` without ``k`` -> float32 [nq, m], the new
        score of every live position in place, +0 at the dead ones.  Asynchronous on the current stream, one launch."""
        torch = _torch()
        head, nq, m, keep = self._rank_call("model_scores_device", model, features, doc, score, count, extra, mode, named_extra)
        with torch.cuda.device(self.device):
            out = torch.empty((nq, m), dtype=torch.float32, device=self.device)
            rc = _capi.lib().srx_ltr_score(*head, _ptr(out), torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(rc, "srx_ltr_score")
        del keep
        return out

    def rank_model(self, model, features, doc, score, count, k: int, extra=None, mode: str = "replace", want_pos: bool = False):
        """Host arrays in (the candidates validated by :func:`~.index.validate_candidates`, ``extra`` a float32 array [nq, m,
        n_extra] or None), host arrays out: :meth:`rank_model_device` with one synchronisation and one copy back."""
        from .ltr import check_mode, resolve_features
        check_mode(mode)
        _, _, n_extra = resolve_features(self.columns, features, model)
        lists = self._host_lists("rank_model", _capi.SRX_LTR_MAX_M, doc, score, count)
        ex = None
        if n_extra:
            if extra is None:
                raise ValueError("rank_model: the features name extra values: give extra [nq, m, n_extra]")
            ex = np.ascontiguousarray(extra, dtype=np.float32)
            if ex.ndim != 3 or ex.shape[:2] != tuple(lists[0].shape):
                raise ValueError("rank_model: extra must be a float32 array [nq, m, n_extra]")
            ex = _torch().as_tensor(ex, device=self.device)
        return self._to_host(self.rank_model_device(model, features, *lists, k, extra=ex, mode=mode, want_pos=want_pos))


def order_has_value(extra: np.ndarray, nulls: str, k: int) -> np.ndarray:
    """bool[rows, k]: which returned entries have a value, from ``extra`` = (count, valued, ..) -- the valueless entries are the
    last ``count - valued`` of a row under "last" / "drop" and the first under "first"."""
    i = np.arange(int(k))[None, :]
    count, valued = extra[:, 0:1], extra[:, 1:2]
    return (i >= count - valued) & (i < count) if nulls == "first" else i < valued


def order_values(col: HostColumn, key: np.ndarray, has: np.ndarray) -> list:
    """``out_key`` words of one row as what a result dict holds: a Python int (int32 / int64), bool, float (float32), the
    dictionary string of a category column, None where ``has`` is False"""
    vals = decode_order_key(col, key).tolist()
    if col.kind == "bool":
        vals = [bool(v) for v in vals]
    elif col.kind == "category":
        vals = [col.dictionary[v] if h else None for v, h in zip(vals, has)]
    return [v if h else None for v, h in zip(vals, has)]
