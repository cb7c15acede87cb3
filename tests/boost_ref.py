"""NumPy restatement of include/boost/sparse_rx_boost.h, written from the header's contract and never from the kernel: fp32
scalars and ``astype`` chains (every operation is its own ufunc call, so nothing is fused), and a stable ``lexsort`` for the cut.

A column is ``(type, data, valid)``: ``data`` an int32 / int64 / float32 array of n_docs entries, ``valid`` a bool array or None.
A clause is a dict with the fields of ``srx_boost_clause`` (``col, flags, origin, inv_step, weight, missing, knot0, n_seg``).
"""
import numpy as np

I32, I64, F32, SET64 = 0, 1, 2, 3
SCORE_MULTIPLY, SCORE_SUM, SCORE_MAX, SCORE_MIN = 0, 1, 2, 3
MULTIPLY, SUM, REPLACE = 0, 1, 2
ABS = 1
MAX_M, MAX_CLAUSES, MAX_COLS, MAX_KNOTS = 2048, 8, 8, 1 << 24
CLAUSE_BYTES = 40
NAN_BITS = 0x7FC00000

CLAUSE_DTYPE = np.dtype([("col", "<i4"), ("flags", "<i4"), ("origin", "<i8"), ("inv_step", "<f4"), ("weight", "<f4"), ("missing", "<f4"),
                         ("knot0", "<i4"), ("n_seg", "<i4"), ("reserved", "<i4")])
f32 = np.float32


def f32_bits(x) -> int:
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def clause_array(clauses) -> np.ndarray:
    """The dicts as the 40-byte records the device reads"""
    out = np.zeros(len(clauses), dtype=CLAUSE_DTYPE)
    for i, c in enumerate(clauses):
        for name in ("col", "flags", "origin", "inv_step", "weight", "missing", "knot0", "n_seg"):
            out[i][name] = c[name]
    return out


def order_map(bits: np.ndarray) -> np.ndarray:
    """uint32 score bits -> int64 that ascends as the score's rank does; every NaN is 0, behind -inf"""
    b = bits.astype(np.uint32)
    m = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.int64)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), 0, m)


def factor(col, clause, knots, local, fused=False) -> np.ndarray:
    """g_c of the header for the local docs ``local`` (all inside the column).  ``fused``: the lerp's multiply-add in float64,
    rounded once -- what a contracted build would compute; only the FMA sensitivity test asks for it."""
    typ, data, valid = col
    n = len(local)
    knots = np.asarray(knots, dtype=np.float32)
    has = np.ones(n, dtype=bool) if valid is None else np.asarray(valid)[local].astype(bool)
    v = np.asarray(data)[local]
    with np.errstate(all="ignore"):
        if typ == F32:
            v = v.astype(np.float32)
            has &= ~np.isnan(v)
            origin = np.array([int(clause["origin"]) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]
            x = (v - origin).astype(np.float32)
        else:
            x = (v.astype(np.int64).astype(np.float64) - np.float64(int(clause["origin"]))).astype(np.float32)
        if int(clause["flags"]) & ABS:
            x = np.abs(x)
        t = (x * f32(clause["inv_step"])).astype(np.float32)
        n_seg = int(clause["n_seg"])
        y = knots[int(clause["knot0"]): int(clause["knot0"]) + n_seg + 1]
        assert len(y) == n_seg + 1 and n_seg >= 1
        low = ~(t > f32(0))
        high = ~low & (t >= f32(n_seg))
        mid = ~low & ~high
        i = np.zeros(n, dtype=np.int64)
        i[mid] = t[mid].astype(np.int32)
        fr = (t - i.astype(np.float32)).astype(np.float32)
        y0, y1 = y[i], y[np.minimum(i + 1, n_seg)]
        dy = (y1 - y0).astype(np.float32)
        if fused:
            lerp = (y0.astype(np.float64) + fr.astype(np.float64) * dy.astype(np.float64)).astype(np.float32)
        else:
            lerp = (y0 + (fr * dy).astype(np.float32)).astype(np.float32)
        f = np.where(low, y[0], np.where(high, y[n_seg], lerp)).astype(np.float32)
        f = np.where(has, f, f32(clause["missing"])).astype(np.float32)
        return (f32(clause["weight"]) * f).astype(np.float32)


def fold(gs, score_mode: int) -> np.ndarray:
    F = gs[0]
    with np.errstate(all="ignore"):
        for g in gs[1:]:
            if score_mode == SCORE_MULTIPLY:
                F = (F * g).astype(np.float32)
            elif score_mode == SCORE_SUM:
                F = (F + g).astype(np.float32)
            elif score_mode == SCORE_MAX:
                F = np.where(g > F, g, F).astype(np.float32)
            else:
                F = np.where(g < F, g, F).astype(np.float32)
    return F


def new_scores(cols, doc_base, clauses, knots, score_mode, boost_mode, doc, score, fused=False) -> np.ndarray:
    """uint32 bits of the new scores of live candidates (global ids ``doc``, raw ``score``)"""
    local = doc.astype(np.int64) - int(doc_base)
    gs = [factor(cols[int(c["col"])], c, knots, local, fused) for c in clauses]
    F = fold(gs, score_mode)
    s = score.astype(np.float32)
    with np.errstate(all="ignore"):
        ns = (s * F).astype(np.float32) if boost_mode == MULTIPLY else (s + F).astype(np.float32) if boost_mode == SUM else F
    bits = ns.view(np.uint32).copy()
    bits[np.isnan(ns)] = NAN_BITS
    return bits


def _live(doc, count, width, n_docs, doc_base):
    n = width if count is None else min(max(int(count), 0), width)
    local = doc[:n].astype(np.int64) - int(doc_base)
    return np.nonzero((local >= 0) & (local < n_docs))[0]


def boost_topk(cols, n_docs, doc_base, clauses, knots, score_mode, boost_mode, cand_doc, cand_score, cand_count, k, carry_doc=None,
               carry_score=None, carry_count=None, fused=False):
    """``srx_boost_topk``: ``(out_doc i32[nq, k], out_score_bits u32[nq, k], out_count i32[nq], out_pos i32[nq, k])``"""
    cand_doc = np.asarray(cand_doc, dtype=np.int32)
    cand_score = np.asarray(cand_score, dtype=np.float32)
    nq, m = cand_doc.shape
    kc = 0 if carry_doc is None else int(np.asarray(carry_doc).shape[1])
    assert 1 <= m and m + kc <= MAX_M and 1 <= k <= m + kc and 1 <= len(clauses) <= MAX_CLAUSES
    out_doc = np.full((nq, k), -1, dtype=np.int32)
    out_bits = np.zeros((nq, k), dtype=np.uint32)
    out_pos = np.full((nq, k), -1, dtype=np.int32)
    out_count = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        docs, bits, pos = [], [], []
        if kc:
            live = _live(np.asarray(carry_doc[q], dtype=np.int32), None if carry_count is None else carry_count[q], kc, n_docs, doc_base)
            docs.append(np.asarray(carry_doc[q], dtype=np.int32)[live])
            bits.append(np.asarray(carry_score[q], dtype=np.float32).view(np.uint32)[live])
            pos.append(live)
        live = _live(cand_doc[q], None if cand_count is None else cand_count[q], m, n_docs, doc_base)
        if len(live):
            docs.append(cand_doc[q][live])
            bits.append(new_scores(cols, doc_base, clauses, knots, score_mode, boost_mode, cand_doc[q][live], cand_score[q][live], fused))
            pos.append(live + kc)
        if not docs:
            continue
        docs, bits, pos = np.concatenate(docs), np.concatenate(bits), np.concatenate(pos)
        order = np.lexsort((docs.astype(np.int64), -order_map(bits)))[:k]  # score descending, then doc ascending
        n = len(order)
        out_doc[q, :n], out_bits[q, :n], out_pos[q, :n], out_count[q] = docs[order], bits[order], pos[order], n
    return out_doc, out_bits, out_count, out_pos


# ---- the fixed-seed data of the bit tests (tests/test_boost_gpu.py; tests/test_boost_cpu.py recomputes it with a fused lerp) -------
N_DOCS, DOC_BASE = 1_000_003, 4096
SPECIAL = 64  # the first local docs hold the planted edge values


def table(seed: int = 7):
    """Three columns of N_DOCS docs -- I32 with a validity row, I64 without, F32 with one -- whose first entries are the edges:
    I64 beyond 2^53 and at both ends of the type, F32 infinities, NaNs (missing), -0.0 and denormals."""
    rng = np.random.default_rng(seed)
    i32 = rng.integers(-50_000, 50_000, N_DOCS).astype(np.int32)
    i64 = rng.integers(1_600_000_000, 1_700_000_000, N_DOCS).astype(np.int64)
    flt = (rng.standard_normal(N_DOCS) * 40).astype(np.float32)
    i32[:6] = [0, -1, 1, 2 ** 31 - 1, -(2 ** 31), 256]
    i64[:10] = [2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 63 - 1, -(2 ** 63), 2 ** 62 + 12345, 0, 1_650_000_000, 1_650_000_000 + 86400, 1_650_000_000 - 1,
                2 ** 53 + 3]
    flt[:12] = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, 3.4028235e38, -3.4028235e38, 1.0, 255.99998],
                        dtype=np.float32)
    flt[12] = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]  # a negative NaN with a payload
    v32 = rng.random(N_DOCS) > 0.1
    vf = rng.random(N_DOCS) > 0.1
    v32[:6], vf[:13] = True, True
    v32[6], vf[13] = False, False
    return [(I32, i32, v32), (I64, i64, None), (F32, flt, vf)]


def curves(rng, n_clauses: int, cols_used=(0, 1, 2), weights=None):
    """``n_clauses`` clauses over random knot tables, cycling through the columns; ``(clauses, knots)``"""
    clauses, knots = [], [np.asarray([0.25], dtype=np.float32)]  # a knot no clause owns in front
    at = 1
    for c in range(n_clauses):
        col = cols_used[c % len(cols_used)]
        n_seg = int(rng.choice([1, 2, 7, 256]))
        y = (rng.random(n_seg + 1) * 1.5 + 0.05).astype(np.float32)
        if col == 0:
            origin, inv = int(rng.integers(-1000, 1000)), f32(n_seg / 60_000.0)
        elif col == 1:
            origin, inv = 1_650_000_000 + int(rng.integers(-10 ** 6, 10 ** 6)), f32(n_seg / 4.0e7)
        else:
            origin, inv = f32_bits(f32(rng.standard_normal() * 5)), f32(n_seg / 90.0)
        w = f32(rng.random() + 0.5) if weights is None else f32(weights[c % len(weights)])
        clauses.append(dict(col=col, flags=int(rng.integers(0, 2)), origin=origin, inv_step=inv, weight=w, missing=f32(rng.random()), knot0=at,
                            n_seg=n_seg))
        knots.append(y)
        at += n_seg + 1
    return clauses, np.concatenate(knots)


def lists(rng, nq: int, m: int, kc: int, special: bool = True):
    """Candidate and carry lists: ids unique per query across carry ++ candidates, a few outside [DOC_BASE, DOC_BASE + N_DOCS) and
    negative, the planted docs among them; counts below 0, inside and above the width."""
    total = m + kc
    doc = np.empty((nq, total), dtype=np.int32)
    for q in range(nq):
        ids = rng.choice(N_DOCS - SPECIAL, size=total, replace=False).astype(np.int64) + SPECIAL + DOC_BASE
        if special:
            n_sp = min(SPECIAL, total // 2)
            ids[rng.choice(total, size=n_sp, replace=False)] = rng.choice(SPECIAL, size=n_sp, replace=False) + DOC_BASE
        for bad in (-1, DOC_BASE - 1, DOC_BASE + N_DOCS, -(2 ** 31), 2 ** 31 - 1, 0):
            if total >= 8 and rng.random() < 0.5:
                ids[int(rng.integers(0, total))] = bad
        doc[q] = ids.astype(np.int32)
    score = (rng.random((nq, total)) * 20 + 0.01).astype(np.float32)

    def counts(width):
        c = rng.integers(max(width // 2, 0), width + 1, nq).astype(np.int32)
        c[rng.random(nq) < 0.15] = width + 5
        if nq > 1:
            c[rng.integers(0, nq)] = -3
        return c
    carry = None if kc == 0 else (np.ascontiguousarray(doc[:, :kc]), np.ascontiguousarray(score[:, :kc]), counts(kc))
    return np.ascontiguousarray(doc[:, kc:]), np.ascontiguousarray(score[:, kc:]), counts(m), carry


def bit_case(seed: int, nq: int = 3, m: int = 257, kc: int = 5, n_clauses: int = 3):
    """One fixed-seed case of the bit tests: ``(clauses, knots, cand_doc, cand_score, cand_count, carry)``"""
    rng = np.random.default_rng(seed)
    clauses, knots = curves(rng, n_clauses)
    return (clauses, knots) + lists(rng, nq, m, kc)
