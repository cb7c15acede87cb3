"""The dense family at scale, as a table: one row per corpus whose rows, tiles, filter bits or score-matrix cells lie on both
sides of a 32-bit boundary of the address arithmetic.  A plain module, as the ``*_ref.py`` files are: it never imports the
package.  tests/test_dense_scale_cpu.py checks the arithmetic of every row with Python integers (the boundary is crossed,
rows are planted on both sides of it, the device bytes stay under the cap); tests/test_dense_scale_gpu.py runs the rows and
nothing else, so the two cannot drift apart.

Construction: the corpus is a zero-filled extent of one device arena; only the PLANTED rows hold values.
A zero row scores exactly 0 and is no result under the searches' ``> 0`` rule, so the expected result of a search is the
ranking of the planted rows alone: O(planted x dim) on the host whatever n_docs is.

Boundaries, in the units the kernels multiply: ``row * dim`` crosses E31 / E32 ELEMENTS, the byte offset behind it B31 / B32
BYTES; a fragment-order layout crosses them with its tile index; the score matrix of a pass crosses them with ``q * ld + d``.

Planted rows for a boundary B: row 0, the last row (tile) that ends at or below B, the row (tile) that straddles B where the
row size does not divide it, the first row (tile) that starts at or above B, row n_docs - 1 and two more rows of the last
partial tile."""
from dataclasses import dataclass

import parity

B31, B32 = 1 << 31, 1 << 32  # bytes
E31, E32 = 1 << 31, 1 << 32  # elements
CAP_BYTES = 24 << 30         # peak device memory of one test: arena + workspace + filter rows
MAX_ID = (1 << 31) - 2       # doc_base + n_docs may be this at most: the returned int32 ids then end at 2^31 - 3
GARBAGE = 0x7F7F7F7F         # what outputs and workspaces hold before a call
GUARD_WORDS = 64             # garbage words behind a workspace that must survive the call
F32_QP = parity.F32_QP

ELEM = {"f32": 4, "u8": 1, "i8": 1, "f16": 2, "bf16": 2, "binary": 1, "tokens": 2}  # bytes per stored element (binary: 8 columns)


def r256(x):
    return (x + 255) // 256 * 256


def pad64(n):
    return (n + 63) // 64 * 64


@dataclass(frozen=True)
class Case:
    name: str
    entries: tuple          # the C entry points the case calls
    kind: str               # key of ELEM
    dim: int
    n_docs: int             # rows of the corpus (tokens: token rows of the store)
    nq: int
    k: int                  # k of a search, m of the binary search
    boundaries: tuple       # names out of B31 B32 E31 E32: on the corpus
    tile: int = 0           # rows per tile of a fragment-order layout the case ALSO or ONLY stores (0: row-major only)
    row_major: bool = True  # the case stores a row-major corpus
    matrix: tuple = ()      # names out of MB32 ME31: on q * ld + d of the INT8 score matrix (4-byte cells)
    n_filters: int = 0      # filter rows the case allocates
    extra_bytes: int = 0    # further device bytes of the case (a second copy of the corpus, scale tables), see `note`
    note: str = ""
    qb: int = 0             # plan cases: the QB the case is written for

    # ---- sizes -------------------------------------------------------------------------------------------------------------
    @property
    def row_bytes(self):
        return self.dim // 8 if self.kind == "binary" else self.dim * ELEM[self.kind]

    @property
    def doc_base_top(self):
        """the largest legal doc_base: doc_base + n_docs == 2^31 - 2"""
        return MAX_ID - self.n_docs

    def boundary_bytes(self, name):
        """byte offset into the corpus at which the named boundary lies"""
        if name in ("B31", "B32"):
            return {"B31": B31, "B32": B32}[name]
        return {"E31": E31, "E32": E32}[name] * ELEM[self.kind]

    def corpus_bytes(self):
        rows = -(-self.n_docs // self.tile) * self.tile if self.tile and not self.row_major else self.n_docs
        return rows * self.row_bytes

    def workspace_bytes(self):
        """the restated `*_workspace_bytes` of the case's search (the GPU test asserts it equals the library's)"""
        n, nq, k = self.n_docs, self.nq, self.k
        if self.kind in ("f32", "u8"):
            return parity.dense_f32_ws_bytes(nq, n, k)
        if self.kind == "i8":
            return parity.dense_ws(nq, n, k)["bytes"]
        if self.kind in ("f16", "bf16"):
            return half_ws_bytes(nq, n, k)
        if self.kind == "binary":
            return binary_ws_bytes(nq, n, k)
        return 0

    def filter_bytes(self):
        return self.n_filters * filter_words(self.n_docs) * 4

    def device_bytes(self):
        """corpus + workspace (with its guard) + filter rows + what `note` names"""
        return self.corpus_bytes() + self.workspace_bytes() + 4 * GUARD_WORDS + self.filter_bytes() + self.extra_bytes

    # ---- planted rows ------------------------------------------------------------------------------------------------------
    def units(self):
        """[(rows per unit, bytes per unit)]: what the layouts of the case index with a 64-bit product"""
        u = [(1, self.row_bytes)] if self.row_major else []
        if self.tile:
            u.append((self.tile, self.tile * self.row_bytes))
        return u

    def planted(self):
        n = self.n_docs
        rows = {0, n - 1}
        for t in (32, 64):  # the last partial tile of 32 and of 64: its first row and the row before the last
            rows.update({n // t * t, n - 2})
        for name in self.boundaries:
            B = self.boundary_bytes(name)
            for per, ub in self.units():
                below, above = B // ub - 1, -(-B // ub)
                idx = {below, above} | ({B // ub} if B % ub else set())
                for u in idx:
                    rows.update({u * per, u * per + per - 1})
        for name in self.matrix:
            for q, d in matrix_cells(self, name):
                rows.update({d - 1, d})
        if self.qb:  # plan cases: the ends of the threshold sample and of the first filter round, and 16 rows spread over the corpus
            p = parity.dense_plan(self.nq, n, self.k, self.dim)
            rows.update({p["S"] - 1, p["S"], p["S1"] - 1, p["S1"]})
            rows.update(i * n // 17 for i in range(1, 17))
        return sorted(r for r in rows if 0 <= r < n)

    def sides(self, name):
        """(planted rows stored wholly below the boundary, planted rows stored wholly at or above it), in every layout"""
        B = self.boundary_bytes(name)
        out = []
        for per, ub in self.units():
            lo = [r for r in self.planted() if (r // per + 1) * ub <= B]
            hi = [r for r in self.planted() if (r // per) * ub >= B]
            out.append((lo, hi))
        return out


def matrix_cells(case, name):
    """(q, d) of the first cell of the pass's score matrix at or past the named boundary, for every row q of the first pass the
    boundary falls into: MB32 = byte 2^32 = cell 2^30, ME31 = cell 2^31 of q * ld + d."""
    M = {"MB32": B32 // 4, "ME31": E31}[name]
    ld = pad64(case.n_docs)
    qb = min(case.nq, parity.dense_qb(case.n_docs))
    return [(q, M - q * ld) for q in range(qb) if 0 < M - q * ld < case.n_docs]


def matrix_last_cell(case):
    """q * ld + d of the last doc of the last query of the first pass"""
    qb = min(case.nq, parity.dense_qb(case.n_docs))
    return (qb - 1) * pad64(case.n_docs) + case.n_docs - 1


def filter_words(n_docs):
    return (-(-n_docs // 32) + 3) // 4 * 4


def half_qb(n_docs):
    return min(max((4 << 30) // (pad64(n_docs) * 4) // 32 * 32, 32), 1024)


def half_ws_bytes(nq, n_docs, k):
    """csrc/half_common.h, half_ws: the packed queries of a pass in whole tiles of 128, its fp32 score matrix, the candidate
    lists (docs, scores, counts) of the row splits, each rounded up to 256 bytes, + 256"""
    qb = min(nq, half_qb(n_docs))
    ns = parity.dense_splits(n_docs, qb, k)
    return r256(-(-qb // 128) * 128 * 1024 * 2) + r256(qb * pad64(n_docs) * 4) + 2 * r256(4 * qb * ns * k) + r256(4 * qb * ns) + 256


def binary_ws_bytes(nq, n_docs, m):
    """include/binary/sparse_rx_binary.h, "The workspace is" """
    ld = pad64(n_docs)
    QB = min(max((1 << 32) // (2 * ld) // 32 * 32, 32), 1024)
    qb = min(nq, QB)
    ns = max(1, min(2048 // max(qb, 1), n_docs // 16384, 4096 // m))
    return r256(2 * qb * ld) + 2 * r256(4 * qb * ns * m) + r256(4 * qb * ns) + r256(4 * qb * m) + 256


TAIL = 77  # rows past the boundary row: 64 + 13, so the last tile of 32 and the last tile of 64 are both partial
_ROWS = ("srx_dense_search_f32", "srx_dense_search_f32_filtered", "srx_dense_score_docs_f32")
_U8 = ("srx_dense_search_u8", "srx_dense_search_u8_filtered", "srx_dense_score_docs_u8")
_I8 = ("srx_dense_search_i8", "srx_dense_pack_i8", "srx_dense_search_i8_packed", "srx_dense_score_docs_i8")
_HALF = ("srx_dense_search_half", "srx_dense_score_docs_half")
_BIN = ("srx_binary_search", "srx_binary_dist_docs")
_LATE = ("srx_maxsim_score_docs_half", "srx_maxsim_rerank_half")


def _n_past(boundary_bytes, row_bytes):
    """rows such that the first row at or above the boundary is followed by TAIL more"""
    return -(-boundary_bytes // row_bytes) + TAIL


CASES = [
    # (a) 8 GiB of f32 rows: byte offsets past 2^31 and 2^32, row * dim past 2^31 elements
    Case("a-f32-1024", _ROWS, "f32", 1024, _n_past(E31 * 4, 4096), 5, 5, ("B31", "B32", "E31"), n_filters=2),
    # (a') rows of 3 072 bytes divide none of the boundaries: a row straddles each
    Case("a-f32-768", _ROWS, "f32", 768, _n_past(E31 * 4, 3072), 5, 5, ("B31", "B32", "E31"), n_filters=2),
    # (b) 16 GiB: row * dim past 2^32 elements, the only case above 8 GiB
    Case("b-f32-1024", _ROWS, "f32", 1024, _n_past(E32 * 4, 4096), 5, 5, ("E31", "E32"), n_filters=2),
    # (c) uint8 rows, 4 GiB.  The scale table is zero-filled too: a zero row de-quantizes to 0 * 0 + 0 and scores +-0, which is not > 0
    Case("c-u8-1024", _U8, "u8", 1024, _n_past(B32, 1024), 5, 5, ("B31", "B32", "E31", "E32"), n_filters=2,
         extra_bytes=8 * _n_past(B32, 1024), note="extra: corpus_scales f32[2 n_docs], zero-filled (scale 0, min 0: a zero row scores 0)"),
    # (d) INT8 rows, 4 GiB row-major AND 4 GiB in fragment order (the pack's output), both live
    Case("d-i8-1024", _I8, "i8", 1024, _n_past(B32, 1024), 5, 5, ("B31", "B32", "E31", "E32"), tile=32,
         extra_bytes=-(-_n_past(B32, 1024) // 32) * 32 * 1024 + 4 * _n_past(B32, 1024),
         note="extra: the packed copy + corpus_scale f32[n_docs]"),
    Case("d-i8-768", _I8, "i8", 768, _n_past(B32, 768), 5, 5, ("B31", "B32", "E31", "E32"), tile=32,
         extra_bytes=-(-_n_past(B32, 768) // 32) * 32 * 768 + 4 * _n_past(B32, 768),
         note="extra: the packed copy + corpus_scale f32[n_docs]; rows and tiles straddle the boundaries"),
    # (e) half rows in fragment order: 4 GiB = 2^31 elements for both types, 8 GiB = 2^32 elements for f16
    Case("e-f16-1024", _HALF, "f16", 1024, _n_past(B32, 2048), 5, 5, ("B31", "E31", "B32"), tile=32, row_major=False, n_filters=2),
    Case("e-bf16-1024", _HALF, "bf16", 1024, _n_past(B32, 2048), 5, 5, ("B31", "E31", "B32"), tile=32, row_major=False, n_filters=2),
    Case("e-f16-1024-8g", _HALF, "f16", 1024, _n_past(E32 * 2, 2048), 5, 5, ("B32", "E32"), tile=32, row_major=False, n_filters=2),
    # (j)'s analogue on the half path, where EVERY query is ranked from the score matrix: QB 32, two passes, 31 x ld >= 2^31
    Case("e-f16-64-2p26", _HALF, "f16", 64, 69_300_013, 33, 5, ("B31", "B32", "E32"), tile=32, row_major=False, matrix=("MB32", "ME31"),
         n_filters=2, qb=0),
    # (f) 1-bit codes, 128 bytes per doc, tiles of 64: the code words past 2^32 bytes.  Three queries: the u16 distance matrix
    # of the pass is 3 x ld x 2 bytes
    Case("f-binary-1024", _BIN, "binary", 1024, _n_past(B32, 128), 3, 16, ("B31", "B32"), tile=64, row_major=False, n_filters=2),
    # (g) MaxSim token rows (f16, dim 128, 256 bytes per token) past 2^32 bytes; docs of 50 tokens, so token ranges start at no tile
    Case("g-tokens-128", _LATE, "tokens", 128, _n_past(B32, 256), 3, 5, ("B31", "B32"), tile=32, row_major=False,
         note="n_docs counts TOKEN rows; docs own 50 token rows each (the last one fewer)"),
]

# (j) the large-corpus branches of the INT8 plan: QB 960, 256 and the floor of 32, nq = QB + 1 (a second pass of one query)
PLAN_CASES = [
    Case("j-qb960", ("srx_dense_search_i8",), "i8", 32, 1_100_013, 961, 10, (), qb=960, extra_bytes=4 * 1_100_013, note="extra: corpus_scale"),
    Case("j-qb256", ("srx_dense_search_i8",), "i8", 32, 4_000_013, 257, 10, (), qb=256, extra_bytes=4 * 4_000_013, note="extra: corpus_scale"),
    # QB 32: 32 x ld x 4 bytes is past 2^32
    Case("j-qb32-2p25", ("srx_dense_search_i8",), "i8", 32, (1 << 25) + TAIL, 33, 10, (), matrix=("MB32",), qb=32,
         extra_bytes=4 * ((1 << 25) + TAIL), note="extra: corpus_scale"),
    # QB 32 and 31 x ld >= 2^31: q * ld alone, not only q * ld + d, leaves int32 in the last row of the pass
    Case("j-qb32-2p26", ("srx_dense_search_i8",), "i8", 32, 69_300_013, 33, 10, ("B31",), matrix=("MB32", "ME31"), qb=32,
         extra_bytes=4 * 69_300_013, note="extra: corpus_scale"),
]

# (h) converters: a chunk of rows whose place in the whole-corpus output lies across byte 2^32.  (entry, kind, dim, rows per tile
# of the output, rows of the chunk).  row0 = the first row of the tile before the one that holds (or starts at) byte 2^32.
CONVERT_CASES = [
    ("srx_dense_quantize_i8", "i8-packed", 768, 32, 64),
    ("srx_dense_quantize_i8", "i8-packed", 1024, 32, 64),
    ("srx_dense_quantize_i8", "i8-rows", 768, 1, 64),
    ("srx_dense_quantize_u8", "u8-rows", 768, 1, 64),
    ("srx_dense_convert_half", "f16", 1024, 32, 64),
    ("srx_dense_convert_half", "bf16", 768, 32, 64),
    ("srx_binary_encode", "binary", 1024, 64, 128),  # tiles of 64 rows: two of them
]
CONVERT_GUARD_TILES = 64


def convert_geometry(kind, dim, tile, n_rows):
    """(row0, n_total, bytes per row of the output, first byte of the chunk's output, one past its last byte)"""
    row_bytes = {"i8-packed": dim, "i8-rows": dim, "u8-rows": dim, "f16": 2 * dim, "bf16": 2 * dim, "binary": dim // 8}[kind]
    unit = max(tile, 32 if kind.endswith("rows") else tile)  # row-major outputs: row0 is free, keep it a multiple of 32
    ub = unit * row_bytes
    first = B32 // ub - (1 if B32 % ub else n_rows // unit // 2)  # the tile before the one holding byte 2^32 / the last tile below it
    row0 = first * unit
    n_total = row0 + n_rows + CONVERT_GUARD_TILES * max(unit, 1) + 13
    return row0, n_total, row_bytes, row0 * row_bytes, (row0 + n_rows) * row_bytes


# (i) filter rows: the last row's first bit index is past 2^32
FILTER_CASE = {"n_docs": (1 << 22) + TAIL, "n_filters": 1025}

ARENA_BYTES = r256(max(c.device_bytes() for c in CASES + PLAN_CASES)) + (1 << 20)
