"""Field predicates on the GPU (include/sparse_rx_fields.h): filter rows built from metadata columns, and the searches that take
them.  Expected bits are never the engine's own: the NumPy restatement (tests/fields_ref.py) on the columns a call was given,
packed as filter rows.  Every comparison is exact -- a bit of a row is right or wrong --, and every output buffer is pre-filled
with 0xFFFFFFFF so that a word the builder does not write shows.  The search tests reuse the environment of
tests/test_filter_gpu.py, with fields synthesised from a seeded generator."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fields_ref  # noqa: E402
import filter_ref  # noqa: E402
from fields_ref import F32, I32, I64, IN, MASK_ALL, MASK_ANY, RANGE, SET64, bits_of_f32 as fb  # noqa: E402
from test_filter_gpu import _FilterEnv, _masks, _search_both  # noqa: E402
from test_gpu_parity import _assert_exact  # noqa: E402
from test_search_plans import CORPORA  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 2048  # docs per workgroup of the builder (csrc/fields.hip, FD_CHUNK_DOCS); rows per batch = chunks // 8, in [1, 16]
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -(2 ** 31), 2 ** 31 - 1, -(2 ** 63), 2 ** 63 - 1
DEVICE = "cuda:0"


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()
    e = _FilterEnv()
    yield e
    for ix in e.indexes.values():
        ix.close()


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


def _records(clauses):
    return np.asarray([[_signed((c & 0xFFFFFFFF) | ((op & 0xFFFFFFFF) << 32)), lo, hi] for c, op, lo, hi in clauses] or np.zeros((0, 3)), dtype=np.int64).reshape(-1, 3)


def _csr(lists):
    import torch
    ptr = np.zeros(len(lists) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in lists])
    ids = np.asarray([c for r in lists for c in r] or [0], np.int32)  # an empty id array still needs an address
    return torch.as_tensor(ptr, device=DEVICE), torch.as_tensor(ids, device=DEVICE)


class _Cols:
    """Columns [(type, data, valid bool[n] or None)] on the device, with the descriptor array of the C call"""

    def __init__(self, cols, n_docs):
        import torch
        import sparse_rx
        from sparse_rx import _capi
        self.cols, self.n_docs, self.keep = cols, n_docs, []
        self.descs = (_capi.FieldColDesc * len(cols))()
        for i, (typ, data, valid) in enumerate(cols):
            assert data.dtype == fields_ref.DTYPES[typ] and data.shape == (n_docs,)
            t = torch.as_tensor(np.ascontiguousarray(data), device=DEVICE)
            v = None if valid is None else torch.as_tensor(sparse_rx.filter.pack_masks(np.asarray(valid, bool)).view(np.int32).reshape(-1).copy(), device=DEVICE)
            self.keep += [t, v]
            self.descs[i].data, self.descs[i].valid, self.descs[i].type = t.data_ptr(), (None if v is None else v.data_ptr()), typ


def _run(dev_cols, clauses, values, all_, any_, none, base=None, q_base=None, stream=None, out=None):
    """Filter rows from the C call as uint32[n_rows, words], the output pre-filled with ones (unless `out` is given)"""
    import torch
    from sparse_rx import _capi
    n_docs = dev_cols.n_docs
    n_rows = len(next(x for x in (all_, any_, none) if x is not None))
    if out is None:
        out = torch.full((n_rows, filter_ref.words(n_docs)), -1, dtype=torch.int32, device=DEVICE)
    rec = torch.as_tensor(_records(clauses), device=DEVICE)
    vals = None if not values else torch.as_tensor(np.asarray([_signed(v & 0xFFFFFFFFFFFFFFFF) for v in values], np.int64), device=DEVICE)
    pairs = [None if x is None else _csr(x) for x in (all_, any_, none)]
    ptrs = [p for pair in pairs for p in ((None, None) if pair is None else (pair[0].data_ptr(), pair[1].data_ptr()))]
    qb = None if q_base is None else torch.as_tensor(np.asarray(q_base, np.int32), device=DEVICE)
    bdesc, keep = (None, None) if base is None else base.launch_args(qb, n_rows)
    s = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()  # the uploads and the fill above ran on the current stream: done before a side stream starts
    rc = _capi.lib().srx_filter_from_fields(0, n_docs, dev_cols.descs, len(dev_cols.cols), rec.data_ptr() if len(clauses) else None, len(clauses),
                                            None if vals is None else vals.data_ptr(), n_rows, *ptrs, bdesc, out.data_ptr(), s.cuda_stream)
    _capi.check(rc, "srx_filter_from_fields")
    s.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _assert_rows(got, masks, label):
    import sparse_rx
    masks = np.asarray(masks, bool)
    exp = sparse_rx.filter.pack_masks(masks)  # the vectorised twin of filter_ref.pack, pinned to it below and in test_terms_cpu.py
    assert np.array_equal(exp[0], filter_ref.pack(masks[0])) and np.array_equal(exp[-1], filter_ref.pack(masks[-1]))
    assert got.shape == exp.shape, label
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{label}: {len(bad)} words differ, first at row {bad[0][0]} word {bad[0][1]}: got {got[tuple(bad[0])]:#x}, expected {exp[tuple(bad[0])]:#x}"


def _lists(rows):
    return tuple([list(r[i]) for r in rows] for i in range(3))


# ---- 1. geometry: every word of every row, tail bits and padding words included ------------------------------------------------------
GEOMETRY = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 2_047, 2_049, 20_011, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 3 * CHUNK + 511, 3 * CHUNK + 513]


def _geometry_cols(n, seed):
    rng = np.random.default_rng(seed)
    d = np.arange(n)
    edge = np.zeros(n, np.int32)  # 1 at the first and the last doc of every chunk, of every wave's 512 docs and of the corpus
    for step in (CHUNK, 512, 64):
        edge[::step] = 1
        edge[step - 1::step] = 1
    edge[[0, n - 1]] = 1
    big = rng.integers(-5, 6, n).astype(np.int64) << 40
    x = rng.uniform(-1, 1, n).astype(np.float32)
    x_ok = rng.random(n) < 0.8
    tags = rng.integers(0, 16, n).astype(np.int64)
    return d, [(I32, edge, None), (I64, big, None), (F32, x, x_ok), (SET64, tags, None)]


@pytest.mark.parametrize("n_docs", sorted(set(GEOMETRY)))
def test_geometry(n_docs):
    import sparse_rx
    d, cols = _geometry_cols(n_docs, n_docs)
    clauses = [(0, RANGE, 1, 1), (1, RANGE, -(2 << 40), 2 << 40), (2, RANGE, fb(-0.5), fb(0.5)), (3, MASK_ANY, 5, 0), (3, MASK_ALL, 3, 0), (1, IN, 0, 2)]
    values = [3 << 40, -(4 << 40)]
    rows = [([0], [], []), ([], [0], []), ([], [], [0]),                                      # one list; the edge clause decides the first and last doc of every chunk
            ([0, 1], [], []), ([1], [2, 3], []), ([2], [], [0]), ([], [3, 5], [4]),           # two lists
            ([1], [0, 2], [4]), ([3, 2], [5, 0, 1], [0, 4]),                                  # three lists
            ([], [], []),                                                                     # the empty triple: every doc
            ([2], [], []), ([], [], [2])]                                                     # a column with a validity row, in all and in none
    all_, any_, none = _lists(rows)
    dev = _Cols(cols, n_docs)
    masks = fields_ref.field_masks(cols, clauses, values, n_docs, all_, any_, none)
    assert masks[0][0] and masks[0][n_docs - 1] and masks[9].all() and not (masks[10] & masks[11]).any()
    if n_docs > CHUNK:
        assert masks[0][CHUNK - 1] and masks[0][CHUNK] and not masks[2][CHUNK]
    _assert_rows(_run(dev, clauses, values, all_, any_, none), masks, f"n_docs={n_docs}")
    _assert_rows(_run(dev, clauses, values, all_, None, None), fields_ref.field_masks(cols, clauses, values, n_docs, all_, None, None), f"n_docs={n_docs} all only")
    _assert_rows(_run(dev, clauses, values, None, None, none), fields_ref.field_masks(cols, clauses, values, n_docs, None, None, none), f"n_docs={n_docs} none only")
    # over a base whose bits at and above n_docs are SET (a row another producer made): they are not docs
    base_masks = _masks(n_docs, [0.5, 1.0], seed=7)
    base_masks[0, [0, n_docs - 1]] = True
    base = sparse_rx.DocFilter.from_masks(base_masks, device=DEVICE)
    q_base = [i % 3 - 1 for i in range(len(rows))]
    got = _run(dev, clauses, values, all_, any_, none, base=base, q_base=q_base)
    _assert_rows(got, fields_ref.field_masks(cols, clauses, values, n_docs, all_, any_, none, base_masks, q_base), f"n_docs={n_docs} with a base")


def test_base_tail_bits_are_not_docs():
    import torch
    import sparse_rx
    n = 100
    d, cols = _geometry_cols(n, 3)
    dev = _Cols(cols, n)
    base = sparse_rx.DocFilter(torch.full((1, filter_ref.words(n)), -1, dtype=torch.int32, device=DEVICE), n)  # every bit set, tail and padding too
    got = _run(dev, [], [], [[]], [[]], [[]], base=base)
    _assert_rows(got, np.ones((1, n), bool), "a base row of all ones")


# ---- 2. values ---------------------------------------------------------------------------------------------------------------------
def test_values():
    n = 333
    rng = np.random.default_rng(11)
    special64 = [I64_MIN, I64_MIN + 1, -(1 << 32), -(1 << 32) + 5, -1, 0, 1, 5, (1 << 32), (1 << 32) + 5, (7 << 32) + 5, I32_MAX, I32_MAX + 1, I32_MIN, I32_MIN - 1,
                 I64_MAX - 1, I64_MAX]
    v64 = np.asarray([special64[i % len(special64)] for i in range(n)], np.int64)
    special32 = [I32_MIN, I32_MIN + 1, -1, 0, 1, 2, I32_MAX - 1, I32_MAX]
    v32 = np.asarray([special32[i % len(special32)] for i in range(n)], np.int32)
    specialf = [np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, 1.17549435e-38, 1.0, -1.0, 3.4028235e38, 0.1]
    vf = np.asarray([specialf[i % len(specialf)] for i in range(n)], np.float32)
    specials = [0, 1, 1 << 63, (1 << 64) - 1, 6, (1 << 63) | 1, 1 << 31, 1 << 32]
    vs = np.asarray([specials[i % len(specials)] for i in range(n)], np.uint64).view(np.int64)
    ok = np.ones(n, bool)
    ok[[0, n - 1, 64, 127]] = False  # the first and the last doc have no value
    cols = [(I32, v32, None), (I64, v64, ok), (F32, vf, None), (SET64, vs, None), (F32, vf, ok)]
    in65 = [int(x) for x in rng.integers(-3, 3, 60)] + [5, 5, (1 << 32) + 5, I64_MIN, I64_MAX]  # 65 values, with duplicates
    values = [(7 << 32) + 5] + in65 + [fb(0.0), fb(np.nan), fb(np.inf), fb(1e-45), fb(0.1), I32_MAX, I32_MIN, 1 << 32]
    F = len(in65) + 1
    clauses = [
        (1, RANGE, 5, 5), (1, RANGE, (1 << 32) + 5, (1 << 32) + 5), (1, RANGE, (1 << 32), (7 << 32) + 4),   # bounds that differ only above bit 32
        (1, RANGE, I64_MIN, I64_MIN), (1, RANGE, I64_MAX, I64_MAX), (1, RANGE, I64_MIN, I64_MAX), (1, RANGE, I64_MIN + 1, I64_MAX - 1),
        (1, RANGE, 6, 5),                                                                                     # lo > hi
        (0, RANGE, I32_MIN, I32_MIN), (0, RANGE, I32_MAX, I32_MAX), (0, RANGE, I64_MIN, I64_MAX), (0, RANGE, I32_MIN - 1, I32_MAX + 1),
        (0, RANGE, I32_MAX + 1, I64_MAX), (0, RANGE, (1 << 32) - 1, (1 << 32) + 1),                           # an I32 value is widened: -1 is not 2^32 - 1
        (1, IN, 0, 0), (1, IN, 0, 1), (1, IN, 1, 65), (0, IN, F + 5, 3),                                      # IN lists of 0, 1 and 65 values; int32 against int64 entries
        (2, RANGE, fb(-0.0), fb(0.0)), (2, RANGE, fb(0.0), fb(np.inf)), (2, RANGE, fb(-np.inf), fb(np.inf)), (2, RANGE, fb(np.nan), fb(np.inf)),
        (2, RANGE, fb(-np.inf), fb(np.nan)), (2, RANGE, fb(1e-45), fb(1e-39)), (2, RANGE, fb(-1e-45), fb(1e-45)), (2, RANGE, fb(1.0), fb(-1.0)),
        (2, RANGE, fb(np.inf), fb(np.inf)), (2, IN, F, 5), (2, IN, F + 1, 1), (4, RANGE, fb(-np.inf), fb(np.inf)),
        (3, MASK_ANY, 0, 0), (3, MASK_ANY, 1, 0), (3, MASK_ANY, I64_MIN, 0), (3, MASK_ANY, -1, 0),            # masks of 0, one bit, bit 63, all ones
        (3, MASK_ALL, 0, 0), (3, MASK_ALL, 1, 0), (3, MASK_ALL, I64_MIN, 0), (3, MASK_ALL, -1, 0), (3, MASK_ALL, I64_MIN | 1, 0),
        # precondition violations the kernel must read as "no doc": ops that do not fit, cols outside the table
        (3, RANGE, I64_MIN, I64_MAX), (3, IN, 0, 1), (0, MASK_ANY, -1, 0), (1, MASK_ALL, 0, 0), (2, MASK_ANY, -1, 0), (1, 4, 0, 0), (1, -1, 0, 0),
        (5, RANGE, I64_MIN, I64_MAX), (-1, RANGE, I64_MIN, I64_MAX), (1 << 20, RANGE, I64_MIN, I64_MAX), (I32_MIN, RANGE, I64_MIN, I64_MAX),
    ]
    nc = len(clauses)
    rows = [([c], [], []) for c in range(nc)] + [([], [], [c]) for c in range(nc)] + [([], [c], []) for c in range(0, nc, 3)]
    rows += [([-1], [], []), ([5, -1], [], []), ([], [-1], []), ([], [-1, 5], []), ([], [], [-1]), ([5], [], [-1, 0]),   # clause id -1 in each list
             ([5, 0], [], [0]), ([5], [5], [5]),                                                                        # a clause in all and in none
             ([5, 5, 10, 5], [16, 16], [7, 7]),                                                                         # duplicates
             ([nc], [], []), ([], [nc + 7], []), ([5], [], [nc]), ([-2], [], []), ([I32_MIN], [], []), ([I32_MAX], [], [])]  # ids outside the table
    all_, any_, none = _lists(rows)
    masks = fields_ref.field_masks(cols, clauses, values, n, all_, any_, none)
    hold = lambda c: masks[c]
    assert hold(0).sum() > 0 and not (hold(0) & hold(1)).any() and hold(2).sum() > 0 and hold(3).sum() > 0 and hold(4).sum() > 0
    assert np.array_equal(hold(5), ok) and not hold(7).any() and hold(10).all() and hold(11).all() and not hold(12).any() and not hold(13).any()
    assert not hold(14).any() and hold(15).sum() > 0 and hold(16).sum() > hold(15).sum() and hold(17).sum() > 0
    assert np.array_equal(hold(18), vf == 0) and np.array_equal(hold(20), ~np.isnan(vf)) and not hold(21).any() and not hold(22).any()
    assert hold(23).sum() > 0 and not hold(25).any() and not hold(30).any() and np.array_equal(hold(34), np.ones(n, bool))
    assert not masks[39:nc].any() and masks[nc:nc + 39].any(axis=1).sum() >= 30
    got = _run(_Cols(cols, n), clauses, values, all_, any_, none)
    _assert_rows(got, masks, "values")


# ---- 3. rows: one, one more than a batch, and more than grid y takes ---------------------------------------------------------------------
def _row_cycle(n_rows):
    triples = [([0], [], []), ([], [1, 2], []), ([], [], [3]), ([0], [2], [1]), ([], [], []), ([-1], [], []), ([3, 0], [], [2])]
    return [triples[r % len(triples)] for r in range(n_rows)], len(triples)


@pytest.mark.parametrize("n_docs,n_rows", [(100, 1), (20_011, 1), (16 * CHUNK + 5, 3), (33 * CHUNK + 5, 5), (130 * CHUNK + 5, 17), (130 * CHUNK + 5, 40), (100, 65_537)])
def test_row_counts(n_docs, n_rows):
    batch = min(16, max(1, ((n_docs + CHUNK - 1) // CHUNK) // 8))
    if n_rows == 40:
        batch = 39  # three batches of 16, the last one partial
    assert n_rows in (1, batch + 1) or (batch == 1 and n_rows > 65_535)  # (100, 65 537): 65 537 batches of one row, grid y = 65 535 and a loop
    d, cols = _geometry_cols(n_docs, 5)
    clauses = [(0, RANGE, 0, 0), (1, RANGE, 0, I64_MAX), (2, RANGE, fb(0.0), fb(1.0)), (3, MASK_ANY, 9, 0)]
    rows, period = _row_cycle(n_rows)
    all_, any_, none = _lists(rows)
    distinct = fields_ref.field_masks(cols, clauses, [], n_docs, *_lists(rows[:period]))
    masks = distinct[np.arange(n_rows) % period]
    got = _run(_Cols(cols, n_docs), clauses, [], all_, any_, none)
    _assert_rows(got, masks, f"n_docs={n_docs} n_rows={n_rows}")


# ---- 4. the base, a side stream, a second call into the same buffer, 32 columns ----------------------------------------------------------
def test_base_stream_and_reuse():
    import torch
    import sparse_rx
    n = 20_011
    d, cols = _geometry_cols(n, 21)
    dev = _Cols(cols, n)
    clauses = [(0, RANGE, 0, 0), (1, RANGE, 0, I64_MAX), (2, RANGE, fb(0.0), fb(1.0)), (3, MASK_ANY, 9, 0)]
    rows, _ = _row_cycle(9)
    all_, any_, none = _lists(rows)
    base_masks = _masks(n, [1.0, 0.5, 0.01], seed=41)
    base = sparse_rx.DocFilter.from_masks(base_masks, device=DEVICE)
    q_base = [(i % 4) - 1 for i in range(len(rows))]  # -1 among them
    exp = fields_ref.field_masks(cols, clauses, [], n, all_, any_, none, base_masks, q_base)
    _assert_rows(_run(dev, clauses, [], all_, any_, none, base=base, q_base=q_base), exp, "3-row base with q_filter")
    exp0 = fields_ref.field_masks(cols, clauses, [], n, all_, any_, none, base_masks[1:], None)
    base1 = sparse_rx.DocFilter.from_masks(base_masks[1:], device=DEVICE)
    _assert_rows(_run(dev, clauses, [], all_, any_, none, base=base1), exp0, "a NULL q_filter: base row 0")
    # a side stream
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    _assert_rows(_run(dev, clauses, [], all_, any_, none, base=base, q_base=q_base, stream=side), exp, "side stream")
    # a second call into the same buffer: other rows, every word rewritten
    out = torch.full((len(rows), filter_ref.words(n)), -1, dtype=torch.int32, device=DEVICE)
    _assert_rows(_run(dev, clauses, [], all_, any_, none, out=out), fields_ref.field_masks(cols, clauses, [], n, all_, any_, none), "first call")
    rev = rows[::-1]
    _assert_rows(_run(dev, clauses, [], *_lists(rev), out=out), fields_ref.field_masks(cols, clauses, [], n, *_lists(rev)), "second call, same buffer")


def test_32_columns_in_one_call():
    n = 4_100
    rng = np.random.default_rng(32)
    cols, clauses = [], []
    for i in range(32):
        typ = (I32, I64, F32, SET64)[i % 4]
        ok = None if i % 3 else rng.random(n) < 0.9
        if typ == F32:
            cols.append((typ, rng.uniform(0, 1, n).astype(np.float32), ok))
            clauses.append((i, RANGE, fb(0.02 * i), fb(1.0)))
        elif typ == SET64:
            cols.append((typ, rng.integers(0, 1 << 20, n).astype(np.int64), ok))
            clauses.append((i, MASK_ANY, 1 << (i % 20), 0))
        else:
            cols.append((typ, rng.integers(0, 100, n).astype(fields_ref.DTYPES[typ]), ok))
            clauses.append((i, RANGE, i, 99))
    rows = [([i], [], []) for i in range(32)] + [([], list(range(32)), []), ([0, 1, 2, 3], [30, 31], [29]), ([], [], [31, 30])]
    all_, any_, none = _lists(rows)
    masks = fields_ref.field_masks(cols, clauses, [], n, all_, any_, none)
    assert all(m.any() for m in masks[:32]) and len({m.tobytes() for m in masks[:32]}) == 32  # every column is told apart
    _assert_rows(_run(_Cols(cols, n), clauses, [], all_, any_, none), masks, "32 columns")


# ---- 5. the Python door --------------------------------------------------------------------------------------------------------------
def _synth_fields(n, seed):
    """Raw field values of n docs and the same as `columns` of FieldTable.from_columns"""
    rng = np.random.default_rng(seed)
    year = rng.integers(1990, 2025, n).astype(np.int32)
    views = rng.integers(0, 1 << 40, n).astype(np.int64)
    price = rng.uniform(0, 100, n).astype(np.float32)
    price_missing = rng.random(n) < 0.1
    src_names = np.asarray(["arxiv", "news", "web", "wiki"])
    src = src_names[rng.integers(0, 4, n)]
    labels = [f"t{i}" for i in range(12)]
    tag_bits = rng.integers(0, 1 << 12, n)
    raw = {"year": [int(v) for v in year], "views": [int(v) for v in views], "price": [None if m else np.float32(v) for v, m in zip(price, price_missing)],
           "src": [str(s) for s in src], "tags": [[labels[i] for i in range(12) if (b >> i) & 1] for b in tag_bits]}
    columns = {"year": year, "views": views, "price": np.ma.masked_array(price, mask=price_missing), "src": raw["src"], "tags": raw["tags"]}
    return raw, columns


def _restated(table, groups, base_masks=None, q_base=None):
    """The masks of `groups` over a FieldTable's host columns: the host resolver's records (pinned to exact arithmetic by
    test_fields_cpu.py) through the restatement"""
    from sparse_rx.fields import WhereResolver
    res = WhereResolver(table.columns)
    for g in groups:
        res.add(g)
    rec, values, lists = res.arrays()
    cols = [(table.columns[c].type, table.columns[c].data, table.columns[c].valid) for c in res.names]
    rows = res.rows
    return fields_ref.field_masks(cols, fields_ref.records(rec), values, table.n_docs, *_lists(rows), base_masks, q_base)


GROUPS = [{"must": [{"field": "year", "gte": 2010}], "should": [{"field": "src", "in": ["wiki", "arxiv", "blog"]}], "must_not": [{"field": "tags", "any_of": ["t3"]}]},
          [{"field": "price", "lt": 50}],
          {"must_not": [{"field": "price", "exists": True}]},
          {"should": [{"field": "views", "gt": 2 ** 39}, {"field": "tags", "all_of": ["t0", "t1"]}, {"field": "src", "eq": "nosuch"}]},
          {},
          {"must": [{"field": "year", "gte": 2000, "lte": 2020.5}, {"field": "price", "gte": 0.1}]}]


def test_python_door():
    import torch
    import sparse_rx
    n = 20_011
    raw, columns = _synth_fields(n, 5)
    table = sparse_rx.FieldTable.from_columns(columns, device=DEVICE, doc_base=77)
    assert table.n_docs == n and table.doc_base == 77 and table.device_bytes() == n * (4 + 8 + 4 + 4 + 8) + filter_ref.words(n) * 4
    assert [table.columns[k].kind for k in columns] == ["int32", "int64", "float32", "category", "set"]
    f = table.filter(GROUPS)
    torch.cuda.synchronize()
    assert isinstance(f, sparse_rx.DocFilter) and (f.n_docs, f.doc_base, f.n_filters) == (n, 77, len(GROUPS))
    masks = _restated(table, GROUPS)
    _assert_rows(f.bits.cpu().numpy().view(np.uint32), masks, "FieldTable.filter")
    # the restated masks agree with the clause dicts evaluated directly on the raw values
    year, price = np.asarray(raw["year"]), fields_ref.where_mask(raw["price"], {"lt": 50})
    assert np.array_equal(masks[1], price) and np.array_equal(masks[2], np.asarray([p is None for p in raw["price"]])) and masks[4].all()
    assert np.array_equal(masks[0], (year >= 2010) & np.isin(raw["src"], ["wiki", "arxiv"]) & ~np.asarray(["t3" in t for t in raw["tags"]]))
    # one group is one row; with a base and q_base
    base_masks = _masks(n, [0.5, 0.1], seed=3)
    base = sparse_rx.DocFilter.from_masks(base_masks, device=DEVICE, doc_base=77)
    q_base = [1, -1, 0, 0, 1, -1]
    g = table.filter(GROUPS, base=base, q_base=q_base)
    torch.cuda.synchronize()
    _assert_rows(g.bits.cpu().numpy().view(np.uint32), _restated(table, GROUPS, base_masks, q_base), "FieldTable.filter with a base")
    one = table.filter(GROUPS[0])
    torch.cuda.synchronize()
    _assert_rows(one.bits.cpu().numpy().view(np.uint32), masks[:1], "one group")
    for bad in (dict(where=GROUPS, q_base=[0] * 6), dict(where=GROUPS, base=base, q_base=[2] * 6), dict(where=GROUPS, base=base, q_base=[0]),
                dict(where=[{"field": "nope", "eq": 1}]), dict(where=GROUPS, base=sparse_rx.DocFilter.from_masks(base_masks, device=DEVICE))):
        with pytest.raises(ValueError):
            table.filter(**bad)
    # the host-array door checks what the device cannot
    rec = np.asarray([[0 | (MASK_ANY << 32), 1, 0]], np.int64)
    with pytest.raises(ValueError, match="does not fit"):
        table.filter_arrays(rec, None, all=(np.asarray([0, 1], np.int32), np.asarray([0], np.int32)))
    table.close()


def test_more_than_32_columns():
    import torch
    import sparse_rx
    n = 1_000
    rng = np.random.default_rng(40)
    columns = {f"c{i}": rng.integers(0, 10, n).astype(np.int32) for i in range(40)}
    table = sparse_rx.FieldTable.from_columns(columns, device=DEVICE)
    where = [{"must": [{"field": "c39", "gte": 5}, {"field": "c3", "lt": 7}]}, {"should": [{"field": f"c{i}", "eq": 0} for i in range(10, 40)]}]
    f = table.filter(where)  # the call passes the 31 columns its clauses name, not the table's 40
    torch.cuda.synchronize()
    exp = np.stack([(columns["c39"] >= 5) & (columns["c3"] < 7), np.any([columns[f"c{i}"] == 0 for i in range(10, 40)], axis=0)])
    _assert_rows(f.bits.cpu().numpy().view(np.uint32), exp, "40-column table")
    with pytest.raises(ValueError, match="at most 32"):
        table.filter({"should": [{"field": f"c{i}", "eq": 0} for i in range(33)]})
    table.close()


# ---- 6. searches under field-built rows = the same searches under from_masks of the restated masks -----------------------------------------
@pytest.mark.parametrize("name", ["uniform", "compact"])
def test_sparse_search_under_field_rows(env, name):
    import sparse_rx
    nq, k = 37, 100
    ix = env.index(name)
    raw, columns = _synth_fields(ix.n_docs, 2024)
    table = sparse_rx.FieldTable.from_columns(columns, device=ix.device, doc_base=ix.doc_base)
    q, full = env.full_ranking(name, nq, "u8", 2001)
    built = table.filter(GROUPS)
    masks = _restated(table, GROUPS)
    restated = sparse_rx.DocFilter.from_masks(masks, device=ix.device, doc_base=ix.doc_base)
    q_filter = np.arange(nq) % (len(GROUPS) + 1) - 1
    ix.set_opts(target_blocks=16)
    try:
        got = _search_both(ix, q, k, built, q_filter)
        exp = _search_both(ix, q, k, restated, q_filter)
    finally:
        ix.set_opts()
    assert (exp[0][2] > 0).all()
    _assert_exact(got[0], exp[0], f"{name} search_device under field rows")
    _assert_exact(got[1], exp[1], f"{name} search_packed_device under field rows")
    # and the rows are the oracle's ranking restricted to the restated sets
    per_query = [None if r < 0 else masks[r] for r in q_filter]
    _assert_exact(got[0], filter_ref.filtered_rows(*full, per_query, CORPORA[name][5].get("doc_base", 0), k), f"{name} against the oracle")
    table.close()


def test_search_past_one_page_under_field_rows(env):
    import sparse_rx
    name, k = "zipf", 1500
    ix = env.index(name)
    raw, columns = _synth_fields(ix.n_docs, 2025)
    table = sparse_rx.FieldTable.from_columns(columns, device=ix.device, doc_base=ix.doc_base)
    group = {"must": [{"field": "year", "gte": 2000}], "must_not": [{"field": "tags", "all_of": ["t0", "t1", "t2"]}]}
    q = env.queries(name, 6, "zipf8", 2002)
    built = table.filter(group)
    restated = sparse_rx.DocFilter.from_masks(_restated(table, [group]), device=ix.device, doc_base=ix.doc_base)
    ix.set_opts(target_blocks=16)
    try:
        got = ix.search(*q, k, filter=built)
        exp = ix.search(*q, k, filter=restated)
    finally:
        ix.set_opts()
    assert (exp[2] > 1024).any(), exp[2].tolist()
    _assert_exact(got, exp, "paged search under field rows")
    table.close()


def test_dense_indexes_under_field_rows():
    import sparse_rx
    n, dim, base = 32_801, 64, 1_000
    rng = np.random.default_rng(52)
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((5, dim)).astype(np.float32)
    raw, columns = _synth_fields(n, 53)
    table = sparse_rx.FieldTable.from_columns(columns, device=DEVICE, doc_base=base)
    groups = GROUPS[:4]
    q_filter = np.array([1, -1, 0, 2, 3], np.int32)
    masks = _restated(table, groups)
    assert all(200 < m.sum() < n for m in masks)
    built = table.filter(groups)
    restated = sparse_rx.DocFilter.from_masks(masks, doc_base=base)
    for dense in (sparse_rx.DenseF32Index(emb, doc_base=base), sparse_rx.DenseHalfIndex(emb, dtype="f16", doc_base=base)):
        for k in (10, 100):
            got = dense.search(queries, k, filter=built, q_filter=q_filter)
            exp = dense.search(queries, k, filter=restated, q_filter=q_filter)
            assert (exp[2] == k).all()
            _assert_exact(got, exp, f"{type(dense).__name__} k={k}")
    table.close()


# ---- 7. the API mirrors on tests/golden/text_small.json ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    import sparse_rx
    ids = list(j["corpus"])
    rng = np.random.default_rng(9)
    meta = {d: {"year": int(rng.integers(2000, 2024)), "src": ["wiki", "arxiv", "web"][i % 3], "tags": [t for t in ("draft", "long", "new") if rng.random() < 0.4]}
            for i, d in enumerate(ids)}
    for d in ids[::7]:
        del meta[d]["year"]  # a doc without a year
    corpus = {d: {**doc, "metadata": meta[d]} for d, doc in j["corpus"].items()}
    tokens = {d: set(sparse_rx.tokenize(doc.get("text", doc.get("content", doc.get("body", ""))) or "")) for d, doc in j["corpus"].items()}
    return j, corpus, meta, tokens


WHERE = {"must": [{"field": "year", "gte": 2008}], "should": [{"field": "src", "in": ["wiki", "arxiv"]}], "must_not": [{"field": "tags", "any_of": ["draft"]}]}


def _keep(meta):
    return [d for d, m in meta.items() if m.get("year") is not None and m["year"] >= 2008 and m["src"] in ("wiki", "arxiv") and "draft" not in m["tags"]]


def _restricted(full, keep, k):
    keep = set(keep)
    return {q: dict([(d, s) for d, s in full[q].items() if d in keep][:k]) for q in full}


def test_api_search_bm25_with_where(text, tmp_path):
    import sparse_rx
    j, corpus, meta, tokens = text
    queries, n_docs, k = j["queries"], len(corpus), 10
    columns = sparse_rx.columns_from_metadata(corpus, ["year", "src", "tags"])
    keep = _keep(meta)
    assert 5 < len(keep) < n_docs // 2
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(corpus)
    with pytest.raises(ValueError, match=r"search_bm25\(where=\.\.\.\) needs the docs' fields"):
        svc.search_bm25(queries, top_k=k, where=WHERE)
    svc.set_doc_fields(columns)
    full = svc.search_bm25(queries, top_k=n_docs)
    n_cached = len(svc.query_cache)
    assert n_cached > 0
    got = svc.search_bm25(queries, top_k=k, where=WHERE)
    exp = _restricted(full, keep, k)
    assert got == exp and [list(got[q]) for q in queries] == [list(exp[q]) for q in queries]
    assert any(len(got[q]) == k for q in queries) and any(got[q] != dict(list(full[q].items())[:k]) for q in queries)
    # the dict form: only the named qids are constrained
    no_year = [d for d, m in meta.items() if "year" not in m]
    got = svc.search_bm25(queries, top_k=k, where={"q1": WHERE, "q2": {"must_not": [{"field": "year", "exists": True}]}})
    for q in queries:
        keep_q = keep if q == "q1" else no_year if q == "q2" else list(meta)
        assert list(got[q].items()) == list(_restricted(full, keep_q, k)[q].items()), q
    # chained: doc filter -> term rows -> field rows
    has_w3 = [d for d in keep if "w3" in tokens[d]]
    shown = has_w3[::2]
    got = svc.search_bm25(queries, top_k=k, where=WHERE, excluded_docs=shown, must_terms=["w3"])
    assert got == _restricted(full, [d for d in has_w3 if d not in set(shown)], k) and any(got.values())
    got = svc.search_bm25(queries, top_k=k, where=WHERE, excluded_docs=shown)
    assert got == _restricted(full, [d for d in keep if d not in set(shown)], k)
    got = svc.search_bm25(queries, top_k=k, where={"q0": WHERE}, must_not_terms={"q0": ["w0"], "q3": ["w1"]}, allowed_docs={"q3": keep[::2], "q4": keep[::3]})
    for q in queries:
        keep_q = ([d for d in keep if "w0" not in tokens[d]] if q == "q0" else [d for d in keep[::2] if "w1" not in tokens[d]] if q == "q3"
                  else keep[::3] if q == "q4" else list(meta))
        assert list(got[q].items()) == list(_restricted(full, keep_q, k)[q].items()), q
    assert svc.search_bm25(queries, top_k=k, where=[{"field": "src", "eq": "blog"}]) == {q: {} for q in queries}  # an unknown category: no doc
    assert svc.search_bm25(queries, top_k=k, where={}) == {q: dict(list(full[q].items())[:k]) for q in queries}
    assert len(svc.query_cache) >= n_cached  # the constrained calls neither read nor wrote the cache (the last one is unconstrained)
    cached = len(svc.query_cache)
    svc.search_bm25(queries, top_k=k, where=WHERE)
    assert len(svc.query_cache) == cached
    r = sparse_rx.OptimizedBM25Retriever(device=DEVICE, tile_log2=6)
    r.build_index_from_corpus(corpus)
    r.set_doc_fields(columns)
    assert r.search(queries, top_k=k, where=WHERE) == exp and len(r.query_cache) == 0
    r.close()
    p = sparse_rx.OptimizedRetriever({"type": "bm25"}, device=DEVICE, tile_log2=6, cache_dir=str(tmp_path))
    p.build_index_from_corpus(corpus)
    p.set_doc_fields(columns)
    pk = p.search(queries, top_k=k, where=WHERE, must_terms=["w3"])
    assert pk == _restricted(p.search(queries, top_k=n_docs), has_w3, k) and any(pk.values())  # its own accumulation order, its own floats
    p.close()
    svc.close()


@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_api_vector_and_hybrid_with_where(text, storage):
    import sparse_rx
    j, corpus, meta, tokens = text
    queries = dict(j["queries"])
    n_docs, dim = len(corpus), 96
    rng = np.random.default_rng(61)
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(corpus)
    svc.set_embeddings(rng.standard_normal((n_docs, dim)).astype(np.float32), storage=storage)
    svc.set_doc_fields(sparse_rx.columns_from_metadata(corpus, ["year", "src", "tags"]))
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    keep = _keep(meta)
    # vector search under a metadata predicate = the same call with the satisfying ids as allowed_docs
    for k, min_score in ((5, 0.0), (len(keep) + 3, -100.0)):
        got = svc.search_by_vector(vecs["q0"], k=k, min_score=min_score, where=WHERE)
        assert got == svc.search_by_vector(vecs["q0"], k=k, min_score=min_score, allowed_docs=keep) and len(got) == min(k, len(keep))
    assert svc.search_by_vector(vecs["q0"], k=5, where=[{"field": "src", "eq": "blog"}]) == []
    # hybrid: both sides get the rows
    for extra in (dict(rescore=True), dict(), dict(mmr_lambda=0.5)):
        got = svc.search_hybrid(queries, vecs, top_k=10, candidates=20, where=WHERE, **extra)
        assert got == svc.search_hybrid(queries, vecs, top_k=10, candidates=20, allowed_docs=keep, **extra), extra
        assert any(got.values()) and all(set(v) <= set(keep) for v in got.values())
    has_w2 = [d for d in keep if "w2" in tokens[d]]
    out = has_w2[::2]
    got = svc.search_hybrid(queries, vecs, top_k=10, candidates=20, where=WHERE, excluded_docs=out, must_terms=["w2"], rescore=True)
    assert got == svc.search_hybrid(queries, vecs, top_k=10, candidates=20, allowed_docs=[d for d in has_w2 if d not in set(out)], rescore=True)
    if storage == "f16":  # late interaction over the field-built rows
        toks = {d: rng.standard_normal((3, 32)).astype(np.float32) for d in corpus}
        svc.set_token_embeddings(toks)
        qt = {q: rng.standard_normal((4, 32)).astype(np.float32) for q in queries}
        got = svc.search_hybrid(queries, vecs, top_k=5, where=WHERE, late_query_tokens=qt)
        assert got == svc.search_hybrid(queries, vecs, top_k=5, allowed_docs=keep, late_query_tokens=qt) and any(got.values())
    assert len(svc.query_cache) == 0
    svc.close()
