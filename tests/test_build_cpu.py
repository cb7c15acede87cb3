"""The index-build kernels' directed inputs, and everything about them that can be checked without a GPU.

tests/test_build_gpu.py imports the tables and generators of this file and compares what csrc/build.hip writes on the MI355X
with tests/build_ref.py bit for bit.  Here: build_ref.layout (vectorised) equals parity.np_build_blocks (the loop form) on every
directed case; every case holds the edges it is named for (edges_of computes them from the arrays, never from the generator's
parameters); the generated term-bound, duplicate and impact inputs have the properties that make them tests; and
srx_auto_unit_tiles, a host function, equals its restatement.

The layout cases.  Postings are placed by a "run ladder": the run of term t in unit u has LADDER[(u + off_t) % 9] postings
(0, 1, 2, 3, 4, 5, 7, 8, 9; capped by the unit's docs), off_t chosen so that terms 0, 1, 2 have an empty run at the first, a
middle and the last unit.  A run's docs are, in this order of preference, the unit's first and last doc, the last doc of its
first tile, the first doc of its second tile, the first doc of its last tile and the doc before it, then others; values are
distinct in every case (half-precision bit patterns counted up from 0x0401, one float32 ulp above them where the index
keeps float32), so a misplaced posting changes bits.  Which case carries which edge:
  tile_log2 6 / 10 / 14                     names tl6-*, tl10-*, tl14-*
  unit_tiles 1, 2, 3                        *-ut1-*, *-ut2-*, *-ut3-*
  unit_tiles = n_tiles, n_tiles + 5         *-utN-*, *-utN5-* (the unit is the whole index / larger than it: one run per term)
  unit_tiles 64                             tl6-ut64-* (4 096 docs, compact copy), tl10-ut64-*, tl14-ut64-* (no compact copy)
  n_docs 1, G - 1, G, G + 1, U, U + 1, 2U + 1   the third name part: d1, dG-1, dG, dG+1, dU, dU+1, d2U+1 (d3G+1 for utN / utN5)
  vocab 1, 64, 65, 130                      v1 (one term), v64, v65, v130 (terms 64 .. 129 share sentinel codes with 0 .. 63)
  runs of 1 / 3 / 4 / 5 from a unit's first doc to its last   every d2U+1 case with ut1 (span3/4/5), every *U+1 case (span1: the
                                            last unit holds one doc)
  a unit of exactly 49 152 docs             tl10-ut48-*, tl14-ut3-dU-*, tl14-ut3-d2U+1-*: local id 49 151 directly under the sentinels' 49 152
  docs 49 151, 49 152, 98 303, 98 304       tl14-ut3-d2U+1-*, tl10-ut48-d2U+1-* (n_docs = 2 x 49 152 + 1) and tl14-ut4-d98305-v130-f32 (no compact
                                            copy: post16 is None and a search still equals the oracle)
  fp16 subnormal, 65 504, 65 520 -> inf, 1e-8 -> +0, -0.0     tl6-ut2-d2U+1-v65-f16-values
  the bits of -0.0, a float32 subnormal, the largest float32  tl10-ut3-dU+1-v64-f32-values"""
import math

import numpy as np
import pytest

import build_ref
from parity import np_build_blocks

LADDER = (0, 1, 2, 3, 4, 5, 7, 8, 9)
F16_VALUES = (2.0 ** -24, 65504.0, 65520.0, 1e-8, -0.0)
F32_VALUES = (-0.0, 1e-45, 3.4028234663852886e38)


class LayoutCase:
    def __init__(self, tile_log2, unit, docs, vocab, vd, edges, special=None):
        self.tile_log2, self.vocab, self.vd, self.edges, self.special = tile_log2, vocab, vd, tuple(edges), special
        G = 1 << tile_log2
        if isinstance(unit, str):  # the unit in terms of the index: n_docs is then given in tiles
            n_docs = {"3G+1": 3 * G + 1}[docs]
            n_tiles = (n_docs + G - 1) // G
            self.unit_tiles = {"N": n_tiles, "N5": n_tiles + 5}[unit]
        else:
            self.unit_tiles = unit
            U = unit * G
            n_docs = docs if isinstance(docs, int) else {"1": 1, "G-1": G - 1, "G": G, "G+1": G + 1, "U": U, "U+1": U + 1, "2U+1": 2 * U + 1}[docs]
        self.n_docs, self.G, self.U = n_docs, G, self.unit_tiles * G
        self.n_tiles = (n_docs + G - 1) // G
        self.n_units = (self.n_tiles + self.unit_tiles - 1) // self.unit_tiles
        self.name = f"tl{tile_log2}-ut{unit}-d{docs}-v{vocab}-{vd}" + ("-values" if special else "")
        self.np_dtype = np.float32 if vd == "f32" else np.float16
        self.score_bounds = special is None
        self._coo = None

    @property
    def coo(self):
        """(rows i32, cols i32, vals f32) sorted by (row, col): the input order DeviceIndex.from_coo takes."""
        if self._coo is None:
            self._coo = _ladder_postings(self)
        return self._coo


def _run_docs(c, t, u, L):
    a, b = u * c.U, min((u + 1) * c.U, c.n_docs)
    last_tile = ((b - 1) >> c.tile_log2) << c.tile_log2
    docs = []
    for d in (a, b - 1, a + c.G - 1, a + c.G, last_tile, last_tile - 1):
        if a <= d < b and d not in docs:
            docs.append(d)
    docs = docs[:L]
    i = 0
    while len(docs) < L:  # 2654435761 is prime and larger than any unit: i -> i * p mod (b - a) visits every doc of the unit
        d = a + (t * 7919 + u * 104729 + i * 2654435761) % (b - a)
        if d not in docs:
            docs.append(d)
        i += 1
    return sorted(docs)


def _ladder_postings(c):
    targets = (0, c.n_units // 2, c.n_units - 1)
    rows, cols = [], []
    for t in range(c.vocab):
        off = (2 * (t // 3) - targets[t % 3]) % 9 if c.vocab >= 3 else 5
        for u in range(c.n_units):
            cap = min((u + 1) * c.U, c.n_docs) - u * c.U
            docs = _run_docs(c, t, u, min(LADDER[(u + off) % 9], cap))
            rows += docs
            cols += [t] * len(docs)
    rows, cols = np.asarray(rows, np.int32), np.asarray(cols, np.int32)  # (term, doc) order
    assert len(rows) < 0x7800 - 0x0401
    vals = (np.arange(len(rows)) + 0x0401).astype(np.uint16).view(np.float16).astype(np.float32)
    if c.vd == "f32":
        vals = np.nextafter(vals, np.float32(np.inf))  # mantissa bits a half cannot hold
    if c.special:
        at = np.arange(len(c.special)) * len(rows) // len(c.special)
        vals[at] = np.asarray(c.special, np.float32)
    o = np.lexsort((cols, rows))
    return rows[o], cols[o], vals[o]


def edges_of(c):
    """The edges a case's ARRAYS hold (see the module docstring), computed without the generator's rules."""
    rows, cols, vals = (np.asarray(x) for x in c.coo)
    r64, c64 = rows.astype(np.int64), cols.astype(np.int64)
    e = {f"tl{c.tile_log2}", f"v{c.vocab}", c.vd}
    if c.unit_tiles in (1, 2, 3, 64):
        e.add(f"ut{c.unit_tiles}")
    if c.unit_tiles == c.n_tiles:
        e.add("unit_is_index")
    if c.unit_tiles > c.n_tiles:
        e.add("unit_gt_index")
    if c.n_tiles == 1:
        e.add("one_tile")
    for name, n in (("1", 1), ("G-1", c.G - 1), ("G", c.G), ("G+1", c.G + 1), ("U", c.U), ("U+1", c.U + 1), ("2U+1", 2 * c.U + 1)):
        if c.n_docs == n:
            e.add("docs=" + name)
    if c.n_docs % c.G:
        e.add("ragged_tile")
    if c.n_tiles % c.unit_tiles:
        e.add("ragged_unit")
    cnt = np.bincount(c64 * c.n_units + r64 // c.U, minlength=c.vocab * c.n_units).reshape(c.vocab, c.n_units)
    if (cnt[:, 0] == 0).any():
        e.add("empty_first")
    if c.n_units >= 3 and (cnt[:, 1:-1] == 0).any():
        e.add("empty_mid")
    if c.n_units >= 2 and (cnt[:, -1] == 0).any():
        e.add("empty_last")
    if (cnt.sum(axis=1) == 0).any():
        e.add("empty_term")
    for t, u in zip(*np.nonzero(cnt)):
        d = r64[(c64 == t) & (r64 // c.U == u)]
        if d.min() == u * c.U and d.max() == min((u + 1) * c.U, c.n_docs) - 1:
            e.add(f"span{len(d)}")
    for L in np.unique(cnt):
        e.add(f"run{L}")
    if (cnt[64:] % 4 != 0).any():
        e.add("sentinel_of_term_64_up")  # padding whose code is (t mod 64), t >= 64
    if (cnt[32:64] % 4 != 0).any():
        e.add("sentinel_of_term_32_up")
    if c.U == 49152 and (r64 % c.U == 49151).any():
        e.add("local_id_49151")
    if {49151, 49152, 98303, 98304} <= set(r64.tolist()):
        e.add("docs_around_49152")
    if c.U > 49152:
        e.add("no_compact")
    if (r64 % c.G == 0).any() and (r64 % c.G == c.G - 1).any():
        e.add("tile_edges")
    with np.errstate(over="ignore"):
        h = vals.astype(np.float16).view(np.uint16)
    fin = np.isfinite(vals)
    for name, hit in (("f16_subnormal", h == 1), ("f16_max", h == 0x7BFF), ("f16_overflow", (h == 0x7C00) & fin),
                      ("f16_underflow", (h == 0) & (vals != 0)), ("neg_zero", vals.view(np.uint32) == 0x80000000),
                      ("f32_subnormal", vals.view(np.uint32) == 1), ("f32_max", vals.view(np.uint32) == 0x7F7FFFFF)):
        if hit.any():
            e.add(name)
    return e


_UNITS3 = ("empty_first", "empty_mid", "empty_last", "tile_edges")
LAYOUT_CASES = [
    # ---- tile_log2 = 6 ----
    LayoutCase(6, 1, "1", 1, "f32", ("one_tile", "docs=1", "span1", "v1")),
    LayoutCase(6, 1, "G-1", 64, "f16", ("one_tile", "docs=G-1", "ragged_tile", "empty_term")),
    LayoutCase(6, 1, "G", 65, "f32", ("docs=G", "docs=U", "sentinel_of_term_64_up", "span9")),
    LayoutCase(6, 1, "G+1", 130, "f32", ("docs=G+1", "docs=U+1", "span1", "sentinel_of_term_64_up", "sentinel_of_term_32_up")),
    LayoutCase(6, 1, "2U+1", 130, "f16", _UNITS3 + ("docs=2U+1", "span1", "span3", "span4", "span5", "run0", "run1", "run3", "run4", "run5")),
    LayoutCase(6, 1, "2U+1", 64, "f32", _UNITS3 + ("span3", "span4", "span5")),
    LayoutCase(6, 2, "U", 64, "f32", ("docs=U", "span4", "tile_edges")),
    LayoutCase(6, 2, "U+1", 65, "f16", ("docs=U+1", "span1", "ragged_unit", "empty_first", "empty_last")),
    LayoutCase(6, 2, "2U+1", 130, "f32", _UNITS3 + ("ragged_unit", "sentinel_of_term_64_up")),
    LayoutCase(6, 2, "G+1", 1, "f16", ("v1", "docs=G+1", "span5")),
    LayoutCase(6, 3, "G+1", 1, "f32", ("v1", "ragged_unit", "span5")),
    LayoutCase(6, 3, "2U+1", 65, "f32", _UNITS3 + ("docs=2U+1", "span1")),
    LayoutCase(6, 3, "U", 130, "f16", ("docs=U", "span3", "sentinel_of_term_64_up")),
    LayoutCase(6, 3, "G-1", 64, "f32", ("one_tile", "unit_gt_index", "docs=G-1")),
    LayoutCase(6, "N", "3G+1", 64, "f32", ("unit_is_index", "ragged_tile", "span5")),
    LayoutCase(6, "N5", "3G+1", 65, "f16", ("unit_gt_index", "span5", "empty_term")),
    LayoutCase(6, 64, "2U+1", 130, "f32", _UNITS3 + ("ut64", "span1")),
    LayoutCase(6, 64, "U+1", 1, "f16", ("ut64", "v1", "span1")),
    LayoutCase(6, 64, "G-1", 64, "f32", ("ut64", "unit_gt_index", "one_tile")),
    LayoutCase(6, 64, "U", 65, "f16", ("ut64", "docs=U", "span4")),
    # ---- tile_log2 = 10 ----
    LayoutCase(10, 1, "1", 130, "f16", ("docs=1", "one_tile", "span1", "empty_term")),
    LayoutCase(10, 1, "2U+1", 65, "f32", _UNITS3 + ("span3", "span4", "span5")),
    LayoutCase(10, 1, "G", 64, "f16", ("docs=G", "one_tile")),
    LayoutCase(10, 2, "G-1", 1, "f32", ("v1", "docs=G-1", "unit_gt_index")),
    LayoutCase(10, 2, "U+1", 130, "f32", ("docs=U+1", "span1", "ragged_unit")),
    LayoutCase(10, 2, "2U+1", 64, "f16", _UNITS3),
    LayoutCase(10, 3, "2U+1", 64, "f16", _UNITS3 + ("ragged_unit",)),
    LayoutCase(10, 3, "G", 65, "f32", ("docs=G", "unit_gt_index")),
    LayoutCase(10, 3, "G+1", 130, "f32", ("docs=G+1", "ragged_unit")),
    LayoutCase(10, "N", "3G+1", 130, "f16", ("unit_is_index", "sentinel_of_term_64_up")),
    LayoutCase(10, "N5", "3G+1", 1, "f32", ("unit_gt_index", "v1")),
    LayoutCase(10, 48, "U", 65, "f32", ("docs=U", "local_id_49151")),
    LayoutCase(10, 48, "2U+1", 130, "f16", _UNITS3 + ("local_id_49151", "docs_around_49152")),
    LayoutCase(10, 64, "U+1", 64, "f32", ("ut64", "no_compact", "span1")),
    # ---- tile_log2 = 14 ----
    LayoutCase(14, 1, "G+1", 65, "f16", ("docs=G+1", "span1")),
    LayoutCase(14, 1, "2U+1", 130, "f32", _UNITS3 + ("span3", "span4", "span5")),
    LayoutCase(14, 1, "G-1", 64, "f32", ("docs=G-1", "one_tile", "ragged_tile")),
    LayoutCase(14, 2, "U", 64, "f32", ("docs=U", "span4")),
    LayoutCase(14, 2, "2U+1", 1, "f16", ("v1", "ragged_unit", "span1")),
    LayoutCase(14, 3, "2U+1", 130, "f32", _UNITS3 + ("local_id_49151", "docs_around_49152", "sentinel_of_term_64_up")),
    LayoutCase(14, 3, "2U+1", 65, "f16", _UNITS3 + ("local_id_49151", "docs_around_49152")),
    LayoutCase(14, 3, "U", 64, "f32", ("docs=U", "local_id_49151")),
    LayoutCase(14, 3, "1", 64, "f16", ("docs=1", "unit_gt_index", "one_tile")),
    LayoutCase(14, 4, 2 * 49152 + 1, 130, "f32", ("no_compact", "docs_around_49152", "ragged_unit")),
    LayoutCase(14, "N", "3G+1", 65, "f16", ("unit_is_index", "no_compact")),
    LayoutCase(14, "N5", "3G+1", 64, "f32", ("unit_gt_index", "no_compact")),
    LayoutCase(14, 64, "U+1", 65, "f32", ("ut64", "no_compact", "span1")),
    # ---- values ----
    LayoutCase(6, 2, "2U+1", 65, "f16", ("f16_subnormal", "f16_max", "f16_overflow", "f16_underflow", "neg_zero"), special=F16_VALUES),
    LayoutCase(10, 3, "U+1", 64, "f32", ("neg_zero", "f32_subnormal", "f32_max"), special=F32_VALUES),
]
LAYOUT_BY_NAME = {c.name: c for c in LAYOUT_CASES}
SEARCHED_CASE = "tl14-ut4-d98305-v130-f32"  # no compact copy: the GPU file also searches it


def coo_to_csr(rows, cols, vals, n_docs):
    indptr = np.zeros(n_docs + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n_docs))
    return indptr, np.asarray(cols, np.int32), np.asarray(vals, np.float32)


def test_case_table_is_sound():
    assert len(LAYOUT_BY_NAME) == len(LAYOUT_CASES) <= 60 and SEARCHED_CASE in LAYOUT_BY_NAME
    have = set().union(*(edges_of(c) for c in LAYOUT_CASES))
    need = {"tl6", "tl10", "tl14", "ut1", "ut2", "ut3", "ut64", "unit_is_index", "unit_gt_index", "v1", "v64", "v65", "v130", "f32", "f16",
            "docs=1", "docs=G-1", "docs=G", "docs=G+1", "docs=U", "docs=U+1", "docs=2U+1", "one_tile", "span1", "span3", "span4", "span5",
            "run0", "run1", "run3", "run4", "run5", "local_id_49151", "docs_around_49152", "no_compact", "f16_subnormal", "f16_max",
            "f16_overflow", "f16_underflow", "neg_zero", "empty_first", "empty_mid", "empty_last", "sentinel_of_term_64_up"}
    assert need <= have, need - have
    for tl in (6, 10, 14):  # 64 tiles per unit at every tile size: with the compact copy where 64 tiles fit it, without elsewhere
        c64 = [c for c in LAYOUT_CASES if c.tile_log2 == tl and c.unit_tiles == 64]
        assert c64 and all((c.U <= 49152) == (tl == 6) for c in c64)


@pytest.mark.parametrize("name", list(LAYOUT_BY_NAME))
def test_layout_case(name):
    """The case holds its edges; build_ref.layout == parity.np_build_blocks bit for bit; every run starts on a multiple of 4 and
    every posting is stored exactly once."""
    c = LAYOUT_BY_NAME[name]
    rows, cols, vals = c.coo
    have = edges_of(c)
    assert set(c.edges) <= have, (name, set(c.edges) - have)
    assert len(np.unique(vals.view(np.uint32))) == len(vals), "values must be distinct"
    with np.errstate(over="ignore"):
        stored = vals.astype(c.np_dtype)
    if not c.special:
        assert len(np.unique(stored)) == len(vals), "values must stay distinct in the index's type"
    assert np.all(np.diff(rows.astype(np.int64) * c.vocab + cols) > 0), "sorted by (row, col), no pair twice"
    tp, post, skip, nb = build_ref.layout(rows, cols, vals, c.n_docs, c.vocab, c.tile_log2, c.unit_tiles, c.np_dtype)
    with np.errstate(over="ignore"):
        e_tp, e_post, e_skip, e_nb = np_build_blocks(*coo_to_csr(rows, cols, vals, c.n_docs), c.n_docs, c.vocab, c.tile_log2, c.unit_tiles, c.np_dtype)
    assert nb == e_nb and np.array_equal(tp, e_tp) and np.array_equal(skip, e_skip)
    assert post.dtype == np.int32 and post.shape == e_post.shape and np.array_equal(post, e_post)
    words = 8 if c.vd == "f32" else 6
    blocks = post.reshape(-1, words)
    docs = blocks[:nb, :4].reshape(-1)
    sk = skip.reshape(c.vocab, c.n_tiles + 1)
    edges = np.minimum(np.arange(c.n_units + 1) * c.unit_tiles, c.n_tiles)
    assert np.all(tp % 4 == 0) and np.all(sk[:, edges] % 4 == 0), "a run's padded start is a multiple of 4"
    real = docs >= 0
    assert real.sum() == len(rows)
    term_of_pos = np.repeat(np.arange(c.vocab), np.diff(tp))
    got_pairs = np.sort(docs[real].astype(np.int64) * c.vocab + term_of_pos[real])
    assert np.array_equal(got_pairs, np.sort(rows.astype(np.int64) * c.vocab + cols)), "every posting exactly once"
    assert np.array_equal(docs[~real], (-1 - 32 * (term_of_pos[~real] % 64)).astype(np.int32))
    assert np.array_equal(blocks[nb:, :4], np.repeat(-1 - 32 * (np.arange(256) % 64), 4).reshape(256, 4)) and not blocks[nb:, 4:].any()
    vbits = blocks[:nb, 4:].copy().view(np.uint32 if c.vd == "f32" else np.uint16).reshape(-1)
    o = np.lexsort((rows, cols))
    assert np.array_equal(vbits[real], stored[o].view(vbits.dtype)), "value bits in (term, doc) order"
    assert not vbits[~real].any(), "a sentinel's value is +0"


# ---- the grid-stride inputs (GPU file: compared in full) ---------------------------------------------------------------------
STRIDE_VOCAB, STRIDE_DOCS, STRIDE_TILE_LOG2, STRIDE_UNIT_TILES = 70_001, 4_000, 6, 5
STRIDE_NNZ = build_ref.CAP_SKIP + 300


def stride_corpus():
    """COO of the index whose skip tables (70 001 x 64 entries) and postings both exceed one trip of the capped grids."""
    rng = np.random.default_rng(20_260)
    cells = np.unique(rng.integers(0, STRIDE_DOCS * STRIDE_VOCAB, STRIDE_NNZ + 200_000))
    cells = cells[np.sort(rng.permutation(len(cells))[:STRIDE_NNZ])]
    assert len(cells) == STRIDE_NNZ
    vals = (rng.random(STRIDE_NNZ, dtype=np.float32) + np.float32(0.5)).astype(np.float32)
    return (cells // STRIDE_VOCAB).astype(np.int32), (cells % STRIDE_VOCAB).astype(np.int32), vals


def test_stride_shapes_cross_the_grid_caps():
    n_tiles = (STRIDE_DOCS + 63) // 64
    assert STRIDE_VOCAB * (n_tiles + 1) == 4_480_064 > build_ref.CAP_SKIP and n_tiles + 1 == 64
    assert n_tiles % STRIDE_UNIT_TILES != 0, "the last unit is partial"
    assert build_ref.CAP_SKIP < STRIDE_NNZ < build_ref.CAP_SKIP + 1000
    assert build_ref.CAP_IMPACT < IMPACT_NNZ < build_ref.CAP_IMPACT + 1000 and IMPACT_NNZ == DUP_GROUPS


IMPACT_NNZ = build_ref.CAP_IMPACT + 300
IMPACT_PARAMS = ((1.2, 0.75, 137.3), (1.6, 0.0, 0.1), (0.9, 1.0, 1.0 / 3.0))  # (k1, b, avgdl): b = 0, b = 1, avgdl no float32


def impact_inputs():
    """(tf f32[nnz], doc i32[nnz], doc_len f32[n]): integer and fractional tf, tf = 0 (only where the doc has a length, so that no
    0 / 0 arises at b = 1), docs of length 0."""
    rng = np.random.default_rng(4_242)
    n = 9_001
    dl = rng.integers(0, 3000, n).astype(np.float32)
    dl[::7] = 0.0
    doc = rng.integers(0, n, IMPACT_NNZ).astype(np.int32)
    tf = rng.integers(1, 40, IMPACT_NNZ).astype(np.float32)
    pick = rng.random(IMPACT_NNZ)
    for lo, v in ((0.00, 0.5), (0.05, 1e-3), (0.10, 1e30), (0.15, 0.0)):
        tf[(pick >= lo) & (pick < lo + 0.05)] = v
    tf[(tf == 0) & (dl[doc] == 0)] = 2.0
    tf[-300:] = np.tile(np.asarray([0.5, 1e-3, 1e30, 3.0, 7.0, 0.25], np.float32), 50)  # the second trip holds every kind too
    return tf, doc, dl


def test_impact_inputs_hold_their_edges():
    from oracle import np_oracle
    tf, doc, dl = impact_inputs()
    for v in (0.5, 1e-3, 1e30, 0.0):
        assert (tf == np.float32(v)).sum() > 1000
    assert (dl[doc] == 0).sum() > 1000 and not ((tf == 0) & (dl[doc] == 0)).any()
    assert any(float(np.float32(a)) != a for _, _, a in IMPACT_PARAMS) and {b for _, b, _ in IMPACT_PARAMS} >= {0.0, 1.0}
    for k1, b, avgdl in IMPACT_PARAMS:
        out = np_oracle.impacts_f32(tf, doc, dl, k1, b, avgdl)
        assert np.isfinite(out).all() and (out[tf == 0] == 0).all()


DUP_GROUPS = build_ref.CAP_IMPACT + 300
DUP_LONG = 4_000


def dup_groups():
    """(first i64[n_groups + 1], vals f32): 2 097 452 groups, 4 000 of them of length 2 .. 9 (some behind the grid's first trip)
    with values whose float32 sum depends on the order: every fourth long group starts with [1e8, 1, -1e8, 1], the rest are random
    mantissas over 12 binades with random signs."""
    rng = np.random.default_rng(77_001)
    n = np.ones(DUP_GROUPS, np.int64)
    long_at = np.sort(rng.choice(DUP_GROUPS - 300, DUP_LONG - 100, replace=False))
    long_at = np.concatenate([long_at, DUP_GROUPS - 300 + np.sort(rng.choice(300, 100, replace=False))])
    n[long_at] = rng.integers(2, 10, DUP_LONG)
    n[long_at[::4]] = np.maximum(n[long_at[::4]], 4)
    first = np.zeros(DUP_GROUPS + 1, np.int64)
    first[1:] = np.cumsum(n)
    vals = (rng.random(first[-1]) + 1.0) * 2.0 ** rng.integers(-6, 6, first[-1])
    vals = (vals * rng.choice([-1.0, 1.0], first[-1])).astype(np.float32)
    for g in long_at[::4]:
        vals[first[g]:first[g] + 4] = (1e8, 1.0, -1e8, 1.0)
    return first, vals, long_at


def test_duplicate_groups_depend_on_the_order():
    first, vals, long_at = dup_groups()
    assert (long_at >= build_ref.CAP_IMPACT).sum() == 100, "long groups in the grid's second trip"
    fwd, rev = build_ref.sum_groups(first, vals), build_ref.sum_groups_reversed(first, vals)
    differs = fwd.view(np.uint32) != rev.view(np.uint32)
    assert not differs[np.diff(first) == 1].any()
    assert differs[long_at].sum() * 2 >= len(long_at), f"only {differs[long_at].sum()} of {len(long_at)} long groups depend on the order"
    assert differs[long_at[long_at >= build_ref.CAP_IMPACT]].sum() >= 40
    g = long_at[0]  # the restatement itself: one rounding per add, left to right
    s = np.float32(vals[first[g]])
    for x in vals[first[g] + 1:first[g + 1]]:
        s = np.float32(s + x)
    assert s.view(np.uint32) == fwd[g].view(np.uint32)
    assert build_ref.sum_groups([0, 4], [1e8, 1.0, -1e8, 1.0])[0] == 1.0 and build_ref.sum_groups_reversed([0, 4], [1e8, 1.0, -1e8, 1.0])[0] == 0.0


def dup_corpus():
    """A doc-major CSR (n_docs, vocab, indptr, cols, vals) in which 300 (doc, term) pairs occur three times, not adjacent in the
    row, with values whose sum depends on the order.  Rows hold at most 12 entries."""
    rng = np.random.default_rng(515)
    n_docs, V = 700, 90
    rows, cols, vals = [], [], []
    trip = set(rng.choice(n_docs, 300, replace=False).tolist())
    for d in range(n_docs):
        ts = rng.choice(V, int(rng.integers(1, 7)), replace=False)
        entries = [(int(t), float(np.float32((rng.random() + 1.0) * 2.0 ** int(rng.integers(-6, 6))))) for t in ts]
        if d in trip:
            t = entries[0][0]
            entries = [(t, 1e8), *entries[1:], (t, 1.0), (t, -1e8)] if d % 2 else \
                [entries[0], *entries[1:], (t, -entries[0][1] * 1024.0), (t, entries[0][1] * 1023.0)]
        rows += [d] * len(entries)
        cols += [t for t, _ in entries]
        vals += [v for _, v in entries]
    rows = np.asarray(rows)
    indptr = np.zeros(n_docs + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n_docs))
    return n_docs, V, indptr, np.asarray(cols, np.int32), np.asarray(vals, np.float32)


def dup_corpus_summed():
    """SciPy's matrix of dup_corpus (it sums duplicates when it assembles a CSR from triples) as sorted COO."""
    from scipy.sparse import csr_matrix
    n_docs, V, indptr, cols, vals = dup_corpus()
    rows = np.repeat(np.arange(n_docs), np.diff(indptr))
    m = csr_matrix((vals, (rows, cols)), shape=(n_docs, V), dtype=np.float32)
    m.sort_indices()
    return m


def test_scipy_sums_the_duplicate_corpus_left_to_right():
    n_docs, V, indptr, cols, vals = dup_corpus()
    assert np.diff(indptr).max() <= 12
    rows = np.repeat(np.arange(n_docs), np.diff(indptr))
    o = np.lexsort((np.arange(len(rows)), cols, rows))  # stable: input order inside a (doc, term) group
    key = rows[o].astype(np.int64) * V + cols[o]
    first = np.concatenate([np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])), [len(key)]])
    assert (np.diff(first) == 3).sum() == 300 and (np.diff(first) > 1).sum() == 300
    fwd, rev = build_ref.sum_groups(first, vals[o]), build_ref.sum_groups_reversed(first, vals[o])
    m = dup_corpus_summed()
    assert m.nnz == len(fwd) and np.array_equal(m.data.view(np.uint32), fwd.view(np.uint32)), "SciPy adds in input order"
    trip = np.diff(first) == 3
    assert (fwd.view(np.uint32) != rev.view(np.uint32))[trip].sum() * 2 >= 300


# ---- term bounds -----------------------------------------------------------------------------------------------------------
TB_VOCAB = 2 * build_ref.TERM_BOUND_GRID + 37
TB_KS_CASES = {"k1": [1], "k1024": [1024], "unsorted": [1000, 1, 1024, 10, 10, 2],
               "nk64": np.random.default_rng(64).choice([1, 2, 3, 5, 10, 64, 100, 255, 256, 257, 1000, 1023, 1024], 64).tolist()}


def tb_stride_inputs(np_dtype):
    """(term_ptr, vals, long terms b): vocab 8 229.  For 300 workgroup indices b: term b has 1 500 .. 5 000 values in [1, 2) (its
    list fills, its threshold ends at >= 1), term b + 4096 has 1 .. 20 values in (0, 0.5), term b + 8192 (b < 37) is empty or all
    zeros.  Every other term has 0 .. 40 values in [0, 2)."""
    rng = np.random.default_rng(8_229)
    grid = build_ref.TERM_BOUND_GRID
    b = np.sort(np.concatenate([np.arange(37), rng.choice(np.arange(37, grid), 263, replace=False)]))
    lens = rng.integers(0, 41, TB_VOCAB)
    lens[b] = rng.integers(1500, 5001, len(b))
    lens[b + grid] = rng.integers(1, 21, len(b))
    lens[np.arange(37) + 2 * grid] = np.where(np.arange(37) % 2, 0, rng.integers(1, 30, 37))
    term_ptr = np.zeros(TB_VOCAB + 1, np.int64)
    term_ptr[1:] = np.cumsum(lens)
    vals = (rng.random(term_ptr[-1]) * 2.0).astype(np.float32)
    vals[rng.random(len(vals)) < 0.1] = 0.0
    for t in b:
        vals[term_ptr[t]:term_ptr[t + 1]] = 1.0 + rng.random(lens[t])
        vals[term_ptr[t + grid]:term_ptr[t + grid + 1]] = 0.001 + 0.49 * rng.random(lens[t + grid])
    for t in np.arange(37) + 2 * grid:
        vals[term_ptr[t]:term_ptr[t + 1]] = 0.0
    return term_ptr, vals.astype(np_dtype), b


def tb_rank_inputs(ks, np_dtype):
    """300 terms with lengths K - 1, K, K + 1 for every K of `ks` (and 0, 1, 2 047), values from a set of 7 (zero included), and,
    per K, a term whose ranks K - 2 .. K + 2 hold one value: ties that straddle rank K."""
    rng = np.random.default_rng(300 + len(ks))
    Ks = sorted(set(ks))
    lens = [0, 1, 2047] + [max(K + d, 0) for K in Ks for d in (-1, 0, 1)]
    lens = np.asarray((lens + [K + 2 for K in Ks] + rng.integers(0, 1100, 300).tolist())[:300], np.int64)
    term_ptr = np.zeros(301, np.int64)
    term_ptr[1:] = np.cumsum(lens)
    vals = rng.choice(np.asarray([0.0, 0.125, 0.25, 0.5, 0.75, 1.5, 3.0], np.float32), term_ptr[-1])
    tie_terms = 3 + 3 * len(Ks) + np.arange(len(Ks))
    for K, t in zip(Ks, tie_terms):
        x = np.concatenate([np.full(max(K - 3, 0), 8.0), np.full(lens[t] - max(K - 3, 0), 4.0)]).astype(np.float32)
        vals[term_ptr[t]:term_ptr[t + 1]] = rng.permutation(x)
    return term_ptr, vals.astype(np_dtype), tie_terms


def test_term_bound_inputs_hold_their_edges():
    grid = build_ref.TERM_BOUND_GRID
    for dt in (np.float32, np.float16):
        term_ptr, vals, b = tb_stride_inputs(dt)
        assert len(term_ptr) - 1 == TB_VOCAB > 2 * grid and len(b) == 300
        exp, neg = build_ref.term_bounds(term_ptr, vals, [1024, 1])
        assert not neg
        # the short term's largest value lies below the long term's 1 024th: a threshold left over from term b hides all of it
        assert np.all(exp[b + grid, 1] > 0) and np.all(exp[b + grid, 1] < exp[b, 0]) and np.all(exp[b, 0] >= 1)
        assert not exp[np.arange(37) + 2 * grid].any()
    for name, ks in TB_KS_CASES.items():
        term_ptr, vals, tie_terms = tb_rank_inputs(ks, np.float32)
        lens = np.diff(term_ptr)
        assert len(lens) == 300 and all({K - 1, K, K + 1} <= set(lens.tolist()) for K in ks)
        for K, t in zip(sorted(set(ks)), tie_terms):
            s = np.sort(vals[term_ptr[t]:term_ptr[t + 1]])[::-1]
            assert s[K - 1] == 4.0 and s[min(K, len(s) - 1)] == 4.0 and (K < 3 or s[K - 2] == 4.0), (name, K)
    assert len(TB_KS_CASES["nk64"]) == 64 and len(set(TB_KS_CASES["nk64"])) < 64 and TB_KS_CASES["nk64"] != sorted(TB_KS_CASES["nk64"])


def test_term_bounds_restatement():
    out, neg = build_ref.term_bounds([0, 3, 3, 7, 9], np.asarray([1, 3, 2, np.nan, 5, np.inf, -0.0, 0.5, -1e-30], np.float32), [1, 2, 3, 3])
    assert np.array_equal(out, np.asarray([[3, 2, 1, 1], [0, 0, 0, 0], [np.inf, 5, 0, 0], [0.5, 0, 0, 0]], np.float32)) and neg
    assert not build_ref.term_bounds([0, 2], np.asarray([-0.0, np.nan], np.float32), [1])[1]


# ---- srx_auto_unit_tiles (a host function: checked here) -------------------------------------------------------------------------
def _auto(n_docs, vocab, nnz, tile_log2):
    from sparse_rx import _capi
    return _capi.lib().srx_auto_unit_tiles(n_docs, vocab, nnz, tile_log2)


def _flip_nnz(n_docs, vocab, tile_log2, t):
    """The largest nnz at which a unit of t + 1 tiles still fits, by bisection on the restatement's own rule."""
    def fits(nnz):
        mean = float(nnz) / (float(n_docs) * float(vocab)) * float(t + 1) * float(1 << tile_log2)
        return mean + 5.0 * math.sqrt(mean) <= 96.0
    lo, hi = 0, n_docs * vocab
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def test_auto_unit_tiles_matches_its_restatement():
    table = [(1, 1, 0, 6), (5, 3, 0, 14), (1_000_000, 50_000, 0, 10)]
    for tl in range(6, 15):
        table += [(1_000_000, 30_000, nnz, tl) for nnz in (40_000, 50_000_000, 3_000_000_000)]  # three densities
    flips = []
    for tl, n_docs, vocab in ((6, 200_000, 5_000), (8, 1_000_003, 997)):
        for t in (1, 2, 3, 63):
            nnz = _flip_nnz(n_docs, vocab, tl, t)
            flips.append((build_ref.auto_unit_tiles(n_docs, vocab, nnz, tl), build_ref.auto_unit_tiles(n_docs, vocab, nnz + 1, tl), t))
            table += [(n_docs, vocab, nnz, tl), (n_docs, vocab, nnz + 1, tl)]
    for below, above, t in flips:  # either side of the density at which fits(t + 1) flips
        assert below == t + 1 and above == t, (below, above, t)
    for n_docs, vocab, nnz, tl in table:
        assert _auto(n_docs, vocab, nnz, tl) == build_ref.auto_unit_tiles(n_docs, vocab, nnz, tl), (n_docs, vocab, nnz, tl)
    got = {tl: build_ref.auto_unit_tiles(5, 3, 0, tl) for tl in range(6, 15)}  # no postings: the largest unit the local ids allow
    assert got == {6: 64, 7: 64, 8: 64, 9: 64, 10: 48, 11: 24, 12: 12, 13: 6, 14: 3}
    assert build_ref.auto_unit_tiles(1000, 10, 10_000, 10) == 1  # every doc holds every term: one tile


def test_auto_unit_tiles_refuses_bad_arguments():
    from sparse_rx import _capi
    for args in ((1000, 10, 100, 5), (1000, 10, 100, 15), (0, 10, 100, 10), (1000, 10, -1, 10), (1000, 0, 100, 10)):
        assert _auto(*args) == -1 and b"srx_auto_unit_tiles" in _capi.lib().srx_last_error(), args
