"""The inputs of the tier-1 route tests, pinned on the CPU.

Tier 1 (csrc/wave_kernel.hip) hands a unit to tier 2 when a term's run does not fit the registers, when the unit needs more
than W_DUPCAP multi-term resolutions, or when it does not fit next to a list of k entries; tier 2 then rescans the unit
exactly, so the final rows cannot tell which tier answered.  tests/parity.py restates the rules (tier1_routes) and the
workspace layout (search_ws); tests/test_tier1_routes_gpu.py reads the flags and the worklist out of the workspace and
compares.  This file builds the directed corpora both files use and asserts, without a GPU, that each one reaches the edge
it was written for: the restated rules give exactly the flagged units the case states, and -- except where a case is
about the list's state (D) -- no unit is left to chance (MAY)."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from parity import item_of, item_queries, plan, plan_workspace_bytes, search_ws, tier1_routes  # noqa: E402

# (mode, val_dtype, build options): BM25 impacts are always fp32; fp16 values exist in dot mode only
VARIANTS = [("bm25", "f32", {}), ("dot", "f32", {"keep_canonical": False}), ("dot", "f16", {})]
VARIANT_IDS = ["bm25-f32", "dot-f32-compact", "dot-f16"]
A_NTS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
B_KINDS = ("two", "eight", "sixtyfour")
E_KS = (1, 10, 11, 100, 101, 112, 113)
F_TARGETS = (6, 9, 12, 2)  # target_blocks that cut a 3-query batch into 2, 3, 4 splits per query and into 2 whole queries + 1 x 2 splits


class Case:
    """One corpus + one query batch + the search it is written for.  flagged = the (query, unit) pairs tier 1 must hand to
    tier 2; every other unit of a query with 0 < nt <= 64 it must serve.  may = the pairs the restated rules leave open
    (case D only; flagged then states what the kernel does, derived in the case's docstring).  The random cases and E state
    no set (flagged = None): there the restated rules are the expectation.  Fields: name, n_docs, vocab, tile_log2, unit_tiles,
    n_super, the CSR (indptr, indices, data, doc_lengths, avgdl), idf, q = (q_ptr, q_term, q_weight), k, debug, doc_base."""


def _make(name, n_docs, vocab, posts, queries, tile_log2, unit_tiles, idf, **kw):
    """posts: (doc, term, value) triples, values fp16-exact; queries: [(terms, weights)] in accumulation order."""
    c = Case()
    p = np.array(sorted((int(d), int(t), float(v)) for d, t, v in posts), dtype=np.float64).reshape(-1, 3)
    docs, terms = p[:, 0].astype(np.int64), p[:, 1].astype(np.int32)
    assert len(set(zip(docs.tolist(), terms.tolist()))) == len(docs), f"{name}: a (doc, term) pair twice"
    assert docs.max(initial=0) < n_docs and terms.max(initial=0) < vocab
    vals = p[:, 2].astype(np.float32)
    assert np.array_equal(vals.astype(np.float16).astype(np.float32), vals), f"{name}: values must be fp16-exact"
    c.name, c.n_docs, c.vocab, c.tile_log2, c.unit_tiles = name, n_docs, vocab, tile_log2, unit_tiles
    c.indptr = np.zeros(n_docs + 1, np.int64)
    c.indptr[1:] = np.cumsum(np.bincount(docs, minlength=n_docs))
    c.indices, c.data = terms, vals
    c.doc_lengths = np.full(n_docs, 8.0, np.float32)  # one length: the BM25 impact is a function of the value alone
    c.avgdl = 8.0
    c.idf = np.asarray(idf, np.float32)
    c.q = _batch(queries)
    c.k, c.debug, c.doc_base = kw.get("k", 10), kw.get("debug", 0), kw.get("doc_base", 0)
    c.flagged, c.may = set(kw.get("flagged", ())), set(kw.get("may", ()))
    c.n_super = (((n_docs + (1 << tile_log2) - 1) >> tile_log2) + unit_tiles - 1) // unit_tiles
    return c


def _batch(queries):
    q_ptr = np.zeros(len(queries) + 1, np.int32)
    q_ptr[1:] = np.cumsum([len(t) for t, _ in queries])
    q_term = np.concatenate([np.asarray(t, np.int32) for t, _ in queries] + [np.zeros(0, np.int32)])
    q_w = np.concatenate([np.asarray(w, np.float32) for _, w in queries] + [np.zeros(0, np.float32)])
    return q_ptr, q_term, q_w


def given_order(q):
    """True when the default oracle (ascending term ids, positive weights only) would not add what the kernel adds."""
    q_ptr, q_term, q_w = q
    for i in range(len(q_ptr) - 1):
        t = q_term[q_ptr[i]:q_ptr[i + 1]]
        if np.any(np.diff(t) < 0) or np.any(q_w[q_ptr[i]:q_ptr[i + 1]] <= 0):
            return True
    return False


LOW = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0)  # ordinary stored values (fp16-exact)


def lpt_of(nt):
    return 64 >> max(0, math.ceil(math.log2(nt)))


# ---- case A: run length ----------------------------------------------------------------------------------------------------
A_LONG, A_FILL = 7, 5


def case_a(nt):
    """One long term with 4 LPT, 4 LPT + 1, 8 LPT, 8 LPT + 1, 12 LPT postings in units 0 .. 4 (served by the NR = 4, 8, 8,
    12, 12 bodies) and 12 LPT + 1 in unit 5 (flagged); unit 6 has no query term, unit 7 only the other terms.  The other
    nt - 1 terms sit in docs of their own with runs of 1 .. 3 postings per unit: every run ends in padding sentinels.  The
    long term's last two postings of a unit carry its largest values (30, 29 in unit 0 down to 20, 19 in unit 5): with the
    term bounds on, tau0 is the contribution of its 10th largest value, so the top 10 come from all five served units and
    every served unit fits next to k entries (no MAY) even at nt = 1, where a unit holds up to 768 single-term docs.
    Up to three queries: the long term in the first, the middle and the last slot."""
    L = lpt_of(nt)
    runs = [4 * L, 4 * L + 1, 8 * L, 8 * L + 1, 12 * L, 12 * L + 1, 0, 0]
    base = 12 * L + 3
    tl = max(6, math.ceil(math.log2(base + 3 * (nt - 1) + 12)))
    U = 1 << tl
    n_docs = 8 * U - 3
    others = [10 + 2 * j for j in range(nt - 1)]
    vocab = 10 + 2 * nt + 2
    posts = []
    for u, run in enumerate(runs):
        for i in range(run):
            v = LOW[(i + u) % len(LOW)]
            if i >= run - 2:
                v = 30.0 - 2 * u - (i - (run - 2))
            posts.append((u * U + i, A_LONG, v))
        if u != 6:
            for j, t in enumerate(others):
                for r in range(1 + (j + u) % 3):
                    posts.append((u * U + base + 3 * j + r, t, LOW[(j + r + u) % len(LOW)]))
        if u >= 6:
            for r in range(3):
                posts.append((u * U + U - 8 + r, A_FILL, 1.0))
    idf = np.full(vocab, 0.5, np.float32)
    idf[A_LONG] = 2.0
    for j, t in enumerate(others):
        idf[t] = 0.3 + 0.01 * j
    queries = []
    for slot in sorted({0, (nt - 1) // 2, nt - 1}):
        terms = others[:slot] + [A_LONG] + others[slot:]
        w = [0.25 * (1 + j % 3) for j in range(nt - 1)]
        queries.append((terms, w[:slot] + [1.5] + w[slot:]))
    c = _make(f"A-nt{nt}", n_docs, vocab, posts, queries, tl, 1, idf, flagged={(q, 5) for q in range(len(queries))})
    c.lpt, c.runs = L, runs
    return c


# ---- case B: multi-term docs -----------------------------------------------------------------------------------------------
B_VALUES = (0.125, 0.5, 1.0, 3.0, 7.0, 12.5, 0.25, 40.0)  # several binades: the fp32 sum depends on the order of its terms


def case_b(kind):
    """Units of 128 docs whose multi-term docs need sum (m - 1) = 0, 48 (served), 49 (flagged), 1 and a few resolution
    visits, in that order: the served 48 and the flagged 49 are neighbours.
      two       : nt = 2, 48 / 49 docs matched by both terms;
      eight     : nt = 8, six docs matched by all eight terms (42 visits) plus 6 / 7 two-term docs; the last unit has a
                  three-term doc next to two-term docs in consecutive ids: a term's block (one lane) holds several docs
                  that need a visit, and the three-term doc's postings sit in three lanes;
      sixtyfour : nt = 64, one doc matched by 49 terms (one entry, 48 visits: served) / by 50 terms (flagged).
    Stored values, idf and weights span several binades; the three queries list the terms ascending, descending and rotated."""
    nt = {"two": 2, "eight": 8, "sixtyfour": 64}[kind]
    U, tl = 128, 7
    terms = [3 + 2 * j for j in range(nt)]
    vocab = 3 + 2 * nt + 1
    if kind == "two":
        units = [[(0,)] * 5 + [(1,)] * 6, [(0, 1)] * 48 + [(0,)] * 3, [(0, 1)] * 49 + [(1,)] * 2, [(0, 1)] + [(0,), (1,)] * 4, [(1,)] * 3]
    elif kind == "eight":
        pairs = [(0, 1), (2, 5), (6, 7), (0, 7), (3, 4), (1, 6), (2, 7)]
        allt = tuple(range(8))
        units = [[(j % 8,) for j in range(20)], [allt] * 6 + pairs[:6] + [(4,), (5,)], [allt] * 6 + pairs[:7] + [(0,)],
                 [(0, 3)] + [(j % 8,) for j in range(9)], [(1, 4, 7), (0, 7), (6, 7), (5, 7), (2,), (3,)]]
    else:
        units = [[(j,) for j in range(64)], [tuple(range(7, 56))] + [(j,) for j in range(0, 64, 5)],
                 [tuple(range(3, 53))] + [(j,) for j in range(1, 64, 7)], [(0, 63)] + [(j,) for j in range(2, 60, 3)],
                 [(5, 6, 60)] + [(j,) for j in range(10, 20)]]
    sums = [sum(len(d) - 1 for d in u) for u in units]
    assert sums[:4] == [0, 48, 49, 1], sums
    posts, n = [], 0
    for u, docs in enumerate(units):
        off = (0, 31, 17, 64, 5)[u]
        assert off + len(docs) <= U
        for i, slots in enumerate(docs):
            for s in slots:
                posts.append((u * U + off + i, terms[s], B_VALUES[(n + s) % len(B_VALUES)]))
                n += 1
    idf = np.full(vocab, 0.4, np.float32)
    w = []
    for j, t in enumerate(terms):
        idf[t] = 0.05 * 1.7 ** (j % 9)
        w.append(2.0 ** ((j % 7) - 3) * (1 + 0.1 * (j % 3)))
    rot = nt // 2
    queries = [(terms, w), (terms[::-1], w[::-1]), (terms[rot:] + terms[:rot], w[rot:] + w[:rot])]
    return _make(f"B-{kind}", 5 * U - 9, vocab, posts, queries, tl, 1, idf, flagged={(q, 2) for q in range(3)})


# ---- case C: id and bitmap edges -------------------------------------------------------------------------------------------
def case_c():
    """Units of 3 x 16 384 = 49 152 docs, 100 001 docs: two full units and a ragged third.  Postings at the local ids 0, 31,
    32 (word edges of the bitmap), 16383, 16384 (a tile edge inside the unit) and 49151 (the last bit of word 1535) of units 0
    and 1 -- doc 49152 is the first doc of the next unit -- and at the first and last doc of unit 2, shared by two and three
    terms.  The terms have t & 63 = 0, 1 and 63: their padding sentinels use the bitmap words 1536, 1537 and 1599.  Nothing
    is flagged.  The index has a doc_base."""
    U = 49152
    sets = {0: (64, 65, 127), 31: (64, 65), 32: (65, 127), 16383: (64, 127), 16384: (64, 65, 127), 49151: (64, 65, 127), 49150: (128,), 7: (191,)}
    posts, n = [], 0
    for u in (0, 1):
        for loc, ts in sets.items():
            for t in ts:
                posts.append((u * U + loc, t, B_VALUES[n % len(B_VALUES)]))
                n += 1
    for d, ts in ((2 * U, (64, 65, 127)), (100_000, (65, 127, 191)), (2 * U + 33, (128, 64))):
        for t in ts:
            posts.append((d, t, B_VALUES[n % len(B_VALUES)]))
            n += 1
    idf = np.full(200, 0.7, np.float32)
    idf[[64, 65, 127, 128, 191]] = (1.3, 0.21, 5.5, 0.9, 2.25)
    queries = [([64, 65, 127], [1.0, 3.5, 0.125]), ([127, 64], [0.75, 2.0]), ([65], [1.0]), ([64, 65, 127, 128, 191], [0.3, 1.0, 2.0, 4.0, 0.6]),
               ([191, 128, 65], [1.0, 1.0, 9.0])]
    return _make("C-edges", 100_001, 200, posts, queries, 14, 3, idf, doc_base=7000)


# ---- case D: the full list -------------------------------------------------------------------------------------------------
def _f16_ramp(n, start=0x3C00):
    return np.arange(start, start + n, dtype=np.uint16).view(np.float16).astype(np.float32)  # n distinct ascending fp16 values from 1.0


def case_d(first):
    """Term bounds off (debug 16: tau0 = 0), one term, k = 10, units of 1 024 docs, the first unit with `first` postings, all
    positive.  From process() of wave_kernel.hip: nt = 1 gives LPT = 64, so 256 postings are 64 blocks, one per lane, one load
    step (NR = 4); the list is empty (count0 = 0), every slot r passes the screen (vthr is the smallest positive float at
    tau = 0) and adds n2 = 64 entries; the test `count + n2 > 256` sees 64, 128, 192, 256: never true, the unit is served with
    the list exactly full.  257 postings are 65 blocks, two steps (NR = 8): slots 0 .. 3 fill the list to 256 and slot 4 brings
    n2 = 1, 257 > 256: U_FULL with nothing to cut (count0 = 0 <= k), so the unit is flagged -- it cannot be redone.  The rules
    of tier1_routes call both units MAY (k + E > 256).  The later units hold five postings each and are served after a cut."""
    U = 1024
    vals = _f16_ramp(first + 10)
    posts = [(i, 9, vals[i]) for i in range(first)]
    posts += [(U + 3 * i, 9, vals[first + i]) for i in range(5)] + [(2 * U + 100 + i, 9, vals[first + 5 + i]) for i in range(5)]
    idf = np.full(12, 1.0, np.float32)
    idf[9] = 1.75
    return _make(f"D-{first}", 3 * U - 7, 12, posts, [([9], [1.0])], 10, 1, idf, debug=16, may={(0, 0)},
                 flagged={(0, 0)} if first > 256 else set())


def case_d_redo():
    """30 units of 128 docs with 100 postings each, values ascending with the doc id, k = 112, term bounds off: every unit
    fits next to k entries (112 + 100 <= 256: MUST_SERVE), the list fills every second unit, is cut to 112 (U_FULL, select)
    and the unit is redone -- again and again, as every later posting beats the threshold."""
    U = 128
    vals = _f16_ramp(3000)
    posts = [(u * U + 11 + i, 4, vals[u * 100 + i]) for u in range(30) for i in range(100)]
    idf = np.full(6, 1.0, np.float32)
    idf[4] = 0.8
    return _make("D-redo", 30 * U, 6, posts, [([4], [1.25])], 7, 1, idf, k=112, debug=16)


# ---- case E: prologue and k ------------------------------------------------------------------------------------------------
def case_e(which):
    """A 2 000-doc uniform corpus in units of 128 docs (k + 128 <= 256 at every k <= 112: no MAY) and one batch mixing
    nt = 0, 1, 2, 3, 5, 8, 9, 17, 64, 65 with empty queries first, in between and last.  `tail`: the last query with terms has
    5 of them, fewer than its NTS = 8 slots, so its scalar prologue takes the branch that repeats the last term instead of
    reading past the arrays; `exact`: the last query has 8 terms and fills its slots exactly.  The 3-term query of `tail` has
    a negative weight (tau0 = 0 for it)."""
    from sparse_rx import synth
    c0 = synth.uniform_corpus_np(2000, 200, 12, seed=91)
    _, idf, avgdl = synth.corpus_stats(c0)
    nts = {"tail": [0, 1, 2, 0, 3, 5, 8, 9, 17, 64, 65, 5, 0], "exact": [0, 1, 2, 0, 3, 5, 9, 17, 64, 65, 0, 8]}[which]
    rng = np.random.default_rng(92 if which == "tail" else 93)
    queries = []
    for nt in nts:
        t = np.sort(rng.choice(200, nt, replace=False)).astype(np.int32)
        w = rng.choice(np.array([0.5, 1.0, 1.0, 2.0, 3.25], np.float32), nt)
        if which == "tail" and nt == 3:
            w[1] = -1.5
        queries.append((t, w))
    c = Case()
    c.name, c.n_docs, c.vocab, c.tile_log2, c.unit_tiles = f"E-{which}", 2000, 200, 7, 1
    c.indptr, c.indices, c.data, c.doc_lengths, c.avgdl, c.idf = c0.indptr, c0.indices, c0.data, c0.doc_lengths, avgdl, idf
    assert np.array_equal(c.data.astype(np.float16).astype(np.float32), c.data)
    c.q, c.k, c.debug, c.doc_base, c.flagged, c.may, c.n_super = _batch(queries), 10, 0, 0, None, set(), 16
    return c


# ---- the random cases ------------------------------------------------------------------------------------------------------
RANDOM = {  # name: (corpus, queries, tile_log2, unit_tiles, k)
    "served": (("uniform", 20_000, 3_000, 30, 73, 1.0), ("uniform", 1.0), 10, 1, 112),
    "flagged": (("zipf", 20_000, 3_000, 40, 72, 1.0), ("zipf", 1.0), 8, 1, 10),
    "mixed": (("zipf", 20_000, 3_000, 40, 72, 0.8), ("zipf", 0.8), 8, 1, 10),  # a flatter zipf: both sets well above 20 %
}


def case_random(name):
    """64 queries of 8 draws (query seed = corpus seed + 100) on a 20 000-doc corpus, default plan, BM25: `served` -- uniform
    terms, 1 024-doc units, k = 112 -- has every pair MUST_SERVE; `flagged` -- zipf(1.0) hot terms, 256-doc units -- has 97 %
    MUST_FLAG; `mixed` -- zipf(0.8), 256-doc units -- 62 % / 38 %.  Units this small leave nothing to the list's state."""
    from sparse_rx import synth
    (kind, n, V, per, seed, s), (qd, qs), tl, ut, k = RANDOM[name]
    c0 = synth.uniform_corpus_np(n, V, per, seed=seed) if kind == "uniform" else synth.zipf_corpus_np(n, V, per, seed=seed, s=s)
    _, idf, avgdl = synth.corpus_stats(c0)
    c = Case()
    c.name, c.n_docs, c.vocab, c.tile_log2, c.unit_tiles = f"R-{name}", n, V, tl, ut
    c.indptr, c.indices, c.data, c.doc_lengths, c.avgdl, c.idf = c0.indptr, c0.indices, c0.data, c0.doc_lengths, avgdl, idf
    c.q = synth.queries_np(64, V, 8, seed=seed + 100) if qd == "uniform" else synth.queries_np(64, V, 8, seed=seed + 100, dist="zipf", s=qs)
    c.k, c.debug, c.doc_base, c.flagged, c.may = k, 0, 0, None, None
    c.n_super = (((n + (1 << tl) - 1) >> tl) + ut - 1) // ut
    return c


# ---- shared by both files --------------------------------------------------------------------------------------------------
def case_plan(c, k=None, target=0):
    nq = len(c.q[0]) - 1
    return plan((c.n_docs + (1 << c.tile_log2) - 1) >> c.tile_log2, c.unit_tiles, nq, c.k if k is None else k, target)


def case_routes(c, p, variant=("bm25", "f32", {}), k=None, debug=None):
    mode, vd, _ = variant
    dbg = c.debug if debug is None else debug
    return tier1_routes(c.indptr, c.indices, c.data, c.doc_lengths, c.idf, c.q, c.tile_log2, c.unit_tiles, c.k if k is None else k, p,
                        term_bound=not (dbg & 16), mode=mode, val_dtype=vd, avgdl=c.avgdl if mode == "bm25" else 1.0)


def expected_bits(c, p, r):
    """The flag bits a directed case states, as bool[items, n_super]: its (query, unit) pairs at the item whose range holds the unit."""
    q_of, _, _ = item_queries(p, len(c.q[0]) - 1)
    exp = np.zeros_like(r["in_range"])
    for q, u in c.flagged:
        exp[:, u] |= (q_of == q) & r["in_range"][:, u]
    return exp


def _check_directed(c, variant, target=0):
    p = case_plan(c, target=target)
    r = case_routes(c, p, variant)
    served_item = ~r["all_t2"] & (r["nt"] > 0)
    assert served_item.all(), f"{c.name}: every query of a directed case is tier 1's"
    exp = expected_bits(c, p, r)
    q_of, _, _ = item_queries(p, len(c.q[0]) - 1)
    may = np.zeros_like(exp)
    for q, u in c.may:
        may[:, u] |= (q_of == q) & r["in_range"][:, u]
    assert np.array_equal(r["may"], may), f"{c.name} {variant[:2]}: MAY units {np.argwhere(r['may'] != may)[:6].tolist()}"
    assert np.array_equal(r["must_flag"], exp & ~may), f"{c.name} {variant[:2]}: MUST_FLAG {np.argwhere(r['must_flag']).tolist()[:8]}"
    assert np.array_equal(r["must_serve"], r["in_range"] & ~exp & ~may), f"{c.name} {variant[:2]}: MUST_SERVE"
    assert exp.sum() == len(c.flagged) and r["in_range"].sum() == (len(c.q[0]) - 1) * c.n_super
    return r


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("nt", A_NTS)
def test_case_a_reaches_every_run_length_edge(nt, variant):
    c = case_a(nt)
    L = lpt_of(nt)
    assert c.runs[:6] == [4 * L, 4 * L + 1, 8 * L, 8 * L + 1, 12 * L, 12 * L + 1] and len(c.q[0]) - 1 == len({0, (nt - 1) // 2, nt - 1})
    # the long term's postings per unit, counted from the CSR itself
    unit_of = np.repeat(np.arange(c.n_docs), np.diff(c.indptr))[c.indices == A_LONG] >> c.tile_log2
    assert np.bincount(unit_of, minlength=8).tolist() == c.runs
    nq = len(c.q[0]) - 1
    for target in (nq, 0) + (F_TARGETS if nq == 3 else ()):  # whole queries, one item per unit, and the split plans of case F
        _check_directed(c, variant, target)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("kind", B_KINDS)
def test_case_b_reaches_48_and_49_resolutions(kind, variant):
    c = case_b(kind)
    for target in (3, 0) + F_TARGETS:
        _check_directed(c, variant, target)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_case_c_and_d_inputs(variant):
    c = case_c()
    r = _check_directed(c, variant)
    assert c.n_super == 3 and not r["must_flag"].any()
    used = {t & 63 for t in c.q[1].tolist()}
    assert {0, 1, 63} <= used
    for first in (256, 257):
        d = case_d(first)
        r = _check_directed(d, variant)
        assert r["may"].sum() == 1 and np.all(r["tau0"] == 0)
        assert int(np.diff(d.indptr)[:1024].sum()) == first
    d = case_d_redo()
    r = _check_directed(d, variant)
    assert r["must_serve"].sum() == 30 and np.all(r["tau0"] == 0)
    assert case_routes(d, case_plan(d), variant, debug=0)["tau0"][0] > 0  # the bounds are what debug bit 16 switches off


@pytest.mark.parametrize("which", ["tail", "exact"])
def test_case_e_inputs(which):
    c = case_e(which)
    q_ptr = c.q[0]
    nts = np.diff(q_ptr)
    assert set(nts.tolist()) == {0, 1, 2, 3, 5, 8, 9, 17, 64, 65} and nts[0] == 0
    last = int(np.flatnonzero(nts)[-1])
    nts_slots = 1 << math.ceil(math.log2(nts[last]))
    assert (q_ptr[last] + nts_slots > q_ptr[-1]) == (which == "tail") and nts_slots == 8
    assert given_order(c.q) == (which == "tail")
    nq = len(nts)
    for k in E_KS:
        for target in (0, 16):
            p = case_plan(c, k, target)
            assert p["n_splits"] == (1 if target else min(16, 4096 // (2 * k)))
            for variant in VARIANTS[:1] if k not in (10, 112) else VARIANTS:
                r = case_routes(c, p, variant, k=k)
                assert not r["may"].any(), f"{c.name} k={k}: MAY units"
                assert r["all_t2"].all() == (k > 112)
                if k <= 112:
                    q_of, _, _ = item_queries(p, nq)
                    assert np.array_equal(r["all_t2"], nts[q_of] > 64)
                    assert r["must_flag"].any() and r["must_serve"].any()
                    neg = [i for i in range(nq) if np.any(c.q[2][q_ptr[i]:q_ptr[i + 1]] < 0)]
                    assert np.all(r["tau0"][neg] == 0) and len(neg) == (which == "tail")


@pytest.mark.parametrize("name", list(RANDOM))
def test_random_cases_land_where_they_should(name):
    c = case_random(name)
    p = case_plan(c)
    r = case_routes(c, p)
    pairs = int(r["in_range"].sum())
    assert pairs == 64 * c.n_super and not r["all_t2"].any()
    nf, ns, nm = int(r["must_flag"].sum()), int(r["must_serve"].sum()), int(r["may"].sum())
    print(f"{c.name}: {pairs} pairs, {nf} MUST_FLAG, {ns} MUST_SERVE, {nm} MAY")
    assert nf + ns + nm == pairs and nm <= 0.05 * pairs
    if name == "served":
        assert (nf, ns, nm) == (0, 1280, 0)
    elif name == "flagged":
        assert (nf, ns, nm) == (4929, 127, 0)
    else:
        assert nf >= 0.2 * pairs and ns >= 0.2 * pairs and (nf, ns, nm) == (3149, 1907, 0)


def test_search_ws_restates_the_workspace_layout():
    """search_ws against plan_workspace_bytes (pinned to srx_search_workspace_bytes by the GPU suites) on every plan shape of
    test_search_plans.CASES, and item_of against decode_item."""
    import test_search_plans as sp
    for name, nq, k, target, _, _ in sp.CASES:
        p = plan(sp._n_tiles(name), sp.UNIT_TILES, nq, k, target)
        w = search_ws(p, nq, k)
        assert w["end"] + 256 == plan_workspace_bytes(p, nq, k), (name, nq, k, target)
        assert w["cand_doc"] == 0 and w["cand_score"] == nq * p["lists_per_q"] * k * 4
        assert w["ovf"] - w["cand_count"] == nq * p["lists_per_q"] * 4 and w["done"] - w["ovf"] == p["items"] * p["ovf_words"] * 4
        assert w["work"] - w["done"] == (nq - p["n_whole"]) * 4 and w["end"] - w["work"] == 4 * (1 + p["items"])
        q_of, split_of, nsq_of = item_queries(p, nq)
        assert [item_of(p, int(q), int(s)) for q, s in zip(q_of, split_of)] == list(range(p["items"]))
        assert np.all(nsq_of[: p["n_whole"]] == 1) and np.all(nsq_of[p["n_whole"]:] == p["n_splits"])
