"""NumPy restatement of include/sparse_rx_fields.h, written from the header: which docs a (must all / must any / must none)
triple of field clauses allows.  Columns are arrays, validity rows bool arrays, clauses (col, op, lo, hi) tuples.  Every compare
is exact: Python ints for the integer and set columns, float64 for float32 columns (a float32 is a float64).  Nothing here calls
the engine; packing the masks into filter rows is filter_ref.pack.  `where_mask` is a second, independent statement: a clause
dict of the Python door evaluated on the column's values in exact arithmetic, for the tests of the host's clause resolution.
Shared by test_fields_cpu.py and test_fields_gpu.py."""
import math

import numpy as np

I32, I64, F32, SET64 = 0, 1, 2, 3
RANGE, IN, MASK_ANY, MASK_ALL = 0, 1, 2, 3
DTYPES = {I32: np.int32, I64: np.int64, F32: np.float32, SET64: np.int64}


def f32_of_bits(x):
    """The float (as a Python float = float64) whose bits are the low 32 of the int64 x"""
    return float(np.asarray(int(x) & 0xFFFFFFFF, dtype=np.uint32).view(np.float32))


def bits_of_f32(f):
    return int(np.asarray(f, dtype=np.float32).view(np.uint32))


def clause_holds(cols, clause, values, n_docs):
    """bool[n_docs]: the docs clause (col, op, lo, hi) holds for.  cols: [(type, data, valid bool[n_docs] or None)]; values: the IN
    lists.  A col outside the list, or an op that does not fit the column's type, holds for no doc."""
    col, op, lo, hi = (int(x) for x in clause)
    none = np.zeros(n_docs, dtype=bool)
    if not (0 <= col < len(cols)):
        return none
    typ, data, valid = cols[col]
    data = np.asarray(data)
    assert data.dtype == DTYPES[typ] and data.shape == (n_docs,)
    if typ in (I32, I64):
        v = data.astype(object)  # Python ints: no width anywhere
        if op == RANGE:
            out = np.asarray([lo <= int(x) <= hi for x in v], dtype=bool)
        elif op == IN:
            member = {int(x) for x in values[lo:lo + max(hi, 0)]}
            out = np.asarray([int(x) in member for x in v], dtype=bool)
        else:
            return none
    elif typ == F32:
        v = data.astype(np.float64)
        if op == RANGE:
            with np.errstate(invalid="ignore"):
                out = (f32_of_bits(lo) <= v) & (v <= f32_of_bits(hi))
        elif op == IN:
            out = none.copy()
            for x in values[lo:lo + max(hi, 0)]:
                out |= v == f32_of_bits(x)  # NaN equals nothing
        else:
            return none
    elif typ == SET64:
        m = lo & 0xFFFFFFFFFFFFFFFF
        v = [int(x) & 0xFFFFFFFFFFFFFFFF for x in data]
        if op == MASK_ANY:
            out = np.asarray([(x & m) != 0 for x in v], dtype=bool)
        elif op == MASK_ALL:
            out = np.asarray([(x & m) == m for x in v], dtype=bool)
        else:
            return none
    else:
        return none
    return out if valid is None else out & np.asarray(valid, dtype=bool)


def field_masks(cols, clauses, values, n_docs, all=None, any=None, none=None, base_masks=None, q_base=None):
    """bool[n_rows, n_docs].  all / any / none: None (no such list) or one list of clause ids per row (-1, or any id outside the
    table: a clause no doc satisfies); base_masks None or bool[n_base, n_docs]; q_base None (base row 0 for every row) or one base
    row per OUTPUT row, -1 = every doc."""
    n_rows = max(len(x) for x in (all, any, none) if x is not None)
    values = [] if values is None else [int(x) for x in values]
    cache = {}

    def holds(c):
        c = int(c)
        if not (0 <= c < len(clauses)):
            return np.zeros(n_docs, dtype=bool)
        if c not in cache:
            cache[c] = clause_holds(cols, clauses[c], values, n_docs)
        return cache[c]

    out = np.ones((n_rows, n_docs), dtype=bool)
    for r in range(n_rows):
        if base_masks is not None:
            b = 0 if q_base is None else int(q_base[r])
            if b >= 0:
                out[r] &= np.asarray(base_masks, dtype=bool).reshape(-1, n_docs)[b]
        for c in (all[r] if all is not None else ()):
            out[r] &= holds(c)
        if any is not None and len(any[r]) > 0:
            one = np.zeros(n_docs, dtype=bool)
            for c in any[r]:
                one |= holds(c)
            out[r] &= one
        for c in (none[r] if none is not None else ()):
            out[r] &= ~holds(c)
    return out


def records(clauses_i64):
    """int64[n, 3] records (col | op << 32, lo, hi) -> [(col, op, lo, hi)]"""
    return [(int(r[0]) & 0xFFFFFFFF, int(r[0]) >> 32, int(r[1]), int(r[2])) for r in np.asarray(clauses_i64).reshape(-1, 3)]


# ---- the Python door's clause dicts, evaluated directly ---------------------------------------------------------------------------
def where_mask(values, clause):
    """bool[n]: a clause dict (gte / gt / lte / lt / eq / in / exists on numbers; eq / in / exists on strings; any_of / all_of /
    exists on collections) on a sequence of values, None = no value, compared in exact arithmetic: Python compares ints and
    floats exactly, and a float32 entry is taken as the float64 it equals."""
    def num(v):
        return float(v) if isinstance(v, (float, np.floating)) else int(v)

    out = []
    for v in values:
        if v is None or (isinstance(v, (float, np.floating)) and math.isnan(float(v)) and "exists" in clause):
            out.append(False)
            continue
        ok = True
        for key, b in clause.items():
            if key == "field":
                continue
            if key == "exists":
                ok &= True
            elif key in ("any_of", "all_of"):
                ok &= (any if key == "any_of" else all)(x in v for x in b) if (key == "all_of" or len(b)) else False
            elif key == "eq":
                ok &= (v == b) if isinstance(v, str) else (num(v) == b)
            elif key == "in":
                ok &= any((v == x) if isinstance(v, str) else (num(v) == x) for x in b)
            else:
                x = num(v)
                ok &= {"gte": x >= b, "gt": x > b, "lte": x <= b, "lt": x < b}[key]
        out.append(bool(ok))
    return np.asarray(out, dtype=bool)
