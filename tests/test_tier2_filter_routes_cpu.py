"""The directed tier-2 cases of tests/test_tier2_routes_cpu.py under doc filters, pinned on the CPU.

A filtered search runs none of the tier-2 instances the other route tests run: csrc/tier2_filter.hip compiles
tier2_kernel.hip a second time, and the filter reaches the candidate sites (hash_unit, flat_tile's two, dense_tile_append,
dense_tile_general's cand_key) through overload resolution alone.  This file builds, from each case and nothing random, the
masks tests/test_tier2_filter_routes_gpu.py runs (masks_for), and asserts without a GPU what makes those runs mean something:

  ones   an all-ones row: the route is the case's own under debug | 8 | 16 (all tier 2, tau0 = 0), step for step;
  knock  results taken away in every tile that holds one: for every step of the route that serves docs, an engine that lost
         the filter inside that step's doc range alone would return other rows (asserted, per step);
  edge   on the upper case of every count pair (1409 / 1408, 1025 / 1024, and 1409 / 1408 behind a search-after bound):
         one filter bit moves the selection to the lower case's outcome, a bit elsewhere does not;
  none   a row of zeros; tail: the ragged last tile alone, its last doc disallowed;
  many_items  1 100 items of one query, more than tier 2's grid of 1 024: a workgroup's second item carries another row.

Expected rows are never the engine's own and never the restatement's: filter_ref.filtered_rows of the oracle's unfiltered
ranking at k = n_docs.  Under every mask the path part of the route (kind, P, M, n_steps, groups, masked, passes) equals the
all-ones route's: the dispatch reads postings, never the mask.

What stays unpinned: the path is restated, never observed.  quads_unit (dense_quads on one flagged unit) cannot occur in a
filtered search -- it is all tier 2, so a query the wave-level dense path can serve takes it over its whole split
(quads_all, the same dense_quads) -- and test_every_step_kind_is_hit asserts that instead of a hit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import filter_ref  # noqa: E402
import parity  # noqa: E402
import test_tier2_routes_cpu as cases  # noqa: E402
from parity import T2_GRID_MAX, plan, tier2_routes  # noqa: E402
from test_tier1_routes_cpu import VARIANTS, VARIANT_IDS, _batch  # noqa: E402

F16_COMPACT = ("dot", "f16", {"keep_canonical": False})  # the instance no other test runs filtered: <__half, compact>
SERVING_KINDS = ("hash", "flat", "quads_all", "packed-hash", "packed-dense", "many_term")
# upper case -> lower case of every count pair
PAIRS = {"S1-1025": "S1-1024", "S1-1409": "S1-1408", "S3-1025": "S3-1024", "S3-1409": "S3-1408", "S1-2433": "S1-2432",
         "S2-many-1025": "S2-many-1024", "S2-1025": "S2-1024", "S4-hash-1025": "S4-hash-1024", "S4-flat-1025": "S4-flat-1024"}
PAGE2_PAIRS = ("S1-2433",)  # the edge lies on the second page of the deep search: after-bound and filter in one predicate
MANY_CASE, MANY_ITEMS = "D1-nt64-nowave", 1100


def case_variants(c):
    """[(id, variant)] the case runs under: its VARIANTS, and the fp16 compact-only form where the search uses the built unit."""
    out = [(VARIANT_IDS[vi], VARIANTS[vi]) for vi in c.variants]
    if not (c.sl or c.override):
        out.append(("dot-f16-compact", F16_COMPACT))
    return out


def nq_of(c):
    return len(c.q[0]) - 1


def full_ranking(c, mode):
    """The oracle's unfiltered ranking of every doc with score > 0 (k = n_docs), once per (case, scoring); never modified."""
    rows = cases.expected_rows(c, mode, k=c.n_docs)
    for a in rows:
        a.setflags(write=False)
    return rows


def per_query(rows, q_filter, nq):
    """The mask of every query: row 0 for all when q_filter is None, else row q_filter[q] (None for -1)."""
    if q_filter is None:
        return [rows[0]] * nq
    return [None if r < 0 else rows[r] for r in q_filter]


def expected(c, mode, rows, q_filter, k=None):
    return filter_ref.filtered_rows(*full_ranking(c, mode), per_query(rows, q_filter, nq_of(c)), c.doc_base, c.k if k is None else k)


_LAYOUT = {}


def routes(c, variant, allowed=None, k=None, after=None, debug=None):
    """tier2_routes of a case with no tier-1 flags (a filtered search leaves nothing to tier 1; neither does debug 8)."""
    mode, vd, _ = variant
    k = c.k if k is None else k
    p = cases.case_plan(c, k)
    key = (c.name, mode, vd)
    if key not in _LAYOUT:
        sv = parity.stored_values(c.indptr, c.data, c.doc_lengths, mode, vd, avgdl=c.avgdl if mode == "bm25" else 1.0)
        _LAYOUT[key] = parity.np_build_blocks(c.indptr, c.indices, sv, c.n_docs, len(c.idf), c.tile_log2, c.unit_tiles)
    return tier2_routes(c.indptr, c.indices, c.data, c.doc_lengths, c.idf, c.q, c.tile_log2, c.unit_tiles, k, p, c.debug if debug is None else debug,
                        np.zeros((p["items"], p["n_super"]), bool), tps=c.tps, mode=mode, val_dtype=vd, avgdl=c.avgdl if mode == "bm25" else 1.0,
                        post16=True, after=after, layout=_LAYOUT[key], allowed=allowed)


def masked_routes(c, variant, rows, q_filter, **kw):
    return routes(c, variant, allowed=per_query(rows, q_filter, nq_of(c)), **kw)


def page2_routes(c, variant, rows, q_filter):
    """The second page of the deep search under a mask: a search-after of k = deep behind the FILTERED first page's last row."""
    ed, es, ec = expected(c, variant[0], rows, q_filter, k=1024)
    assert np.all(ec == 1024), f"{c.name}: the filtered first page is not full"
    return masked_routes(c, variant, rows, q_filter, k=c.deep, after=(es[:, 1023], ed[:, 1023] - c.doc_base))


# ---- reading a route ---------------------------------------------------------------------------------------------------------
def path_part(steps):
    """The steps without what a filter may change (selection outcomes, `compact`, emit's count)."""
    out = []
    for s in steps:
        if s[0] == "many_term":
            out.append(s[:5])
        elif s[0] == "quads_all":
            out.append(s[:4])
        elif s[0] == "emit":
            out.append(("emit",))
        elif s[0] in ("skip", "t1_fold"):
            out.append((s[0],))
        elif s[1] in ("empty", "flat_refused"):
            out.append(tuple(s))
        elif s[1] in ("flat", "hash"):
            out.append(s[:4])
        elif s[1] == "quads_unit":
            out.append(s[:5])
        else:
            assert s[1] == "packed", s
            out.append((s[0], "packed", [g[:3] for g in s[2]]))
    return out


def outcomes(steps):
    """Every selection outcome (name, n) of an item in the order the kernel decides them: the order of sel_docs."""
    out = []
    for s in steps:
        if s[0] == "many_term":
            out += list(s[5])
        elif s[0] == "quads_all":
            out += list(s[4])
        elif s[0] in ("emit", "skip"):
            continue
        elif s[0] == "t1_fold":
            raise AssertionError("tier 1 serves nothing in a filtered search")
        elif s[1] == "flat":
            out += list(s[4])
        elif s[1] == "hash":
            out.append(s[4])
        elif s[1] == "quads_unit":
            out += list(s[5])
        elif s[1] == "packed":
            out += [g[3] for g in s[2] if g[2] != "empty"]
    return out


def compacts(steps):
    return [s[-1] for s in steps if s[0] == "quads_all"]


def serving_steps(c, steps):
    """(kind, lo, hi, label) of every step that forms candidates: the docs [lo, hi) it serves."""
    G, tps = 1 << c.tile_log2, c.tps
    rng = lambda ja, jb: (ja * G, min(jb * G, c.n_docs))  # noqa: E731
    out = []
    for s in steps:
        if s[0] in ("many_term", "quads_all"):
            out.append((s[0],) + rng(s[1], s[2]) + (f"{s[0]} tiles {s[1]}:{s[2]}",))
        elif s[0] in ("emit", "skip", "t1_fold") or s[1] in ("empty", "flat_refused"):
            continue
        elif s[1] in ("flat", "hash"):
            out.append((s[1],) + rng(s[0] * tps, min(s[0] * tps + tps, c.n_tiles)) + (f"{s[1]} unit {s[0]}",))
        elif s[1] == "quads_unit":
            out.append((s[1],) + rng(s[2], s[3]) + (f"quads_unit {s[0]}",))
        else:
            for tiles, GP, kind, _ in s[2]:
                if kind != "empty":
                    out.append(("packed-" + kind,) + rng(*tiles) + (f"packed unit {s[0]} tiles {tiles}",))
    return out


# ---- the masks ---------------------------------------------------------------------------------------------------------------
def result_docs(c, mode):
    """T: the local docs of the oracle's rows at k, over all queries of the case (the all-ones result)."""
    ed, es, ec = cases.expected_rows(c, mode)
    return np.unique(np.concatenate([ed[q, :ec[q]].astype(np.int64) - c.doc_base for q in range(len(ec))]))


def knock_mask(c, mode):
    """Allowed docs of `knock`: every second doc of T (in doc order) is disallowed, and one more where a tile's docs of T would
    all stay; so are doc n_docs - 1 and the first and last doc of every tile that holds a doc of T."""
    T = result_docs(c, mode)
    G = 1 << c.tile_log2
    m = np.ones(c.n_docs, bool)
    m[T[::2]] = False
    for j in np.unique(T >> c.tile_log2):
        in_tile = T[(T >> c.tile_log2) == j]
        if m[in_tile].all():
            m[in_tile[0]] = False
        m[j * G] = False
        m[min(j * G + G, c.n_docs) - 1] = False
    m[c.n_docs - 1] = False
    return m


def tail_mask(c):
    G = 1 << c.tile_log2
    assert c.n_docs % G, f"{c.name}: the last tile is not ragged"
    m = np.zeros(c.n_docs, bool)
    m[(c.n_tiles - 1) * G:] = True
    m[c.n_docs - 1] = False
    return m


def edge_site(name, variant):
    """The selection step an upper case was written for, in the FILTERED restatement under an all-ones row: (page2, item, i,
    upper outcome, lower outcome, group), i = the index into outcomes(steps) of the first outcome that differs from the lower
    case's, group = the docs that decision counted (those on the list and the candidates)."""
    up, lo = cases.get_case(name), cases.get_case(PAIRS[name])
    page2 = name in PAGE2_PAIRS
    ones_u, ones_l = np.ones((1, up.n_docs), bool), np.ones((1, lo.n_docs), bool)
    ru = page2_routes(up, variant, ones_u, None) if page2 else masked_routes(up, variant, ones_u, None)
    rl = page2_routes(lo, variant, ones_l, None) if page2 else masked_routes(lo, variant, ones_l, None)
    assert len(ru["steps"]) == len(rl["steps"]) == 1
    ou, ol = outcomes(ru["steps"][0]), outcomes(rl["steps"][0])
    assert [x[0] for x in ru["sel_docs"][0]] == ou, f"{name}: the decisions' log is not in step order"
    assert len(ou) == len(ol) and ou != ol, f"{name}: the pair's routes do not differ: {ou}"
    i = next(n for n in range(len(ou)) if ou[n] != ol[n])
    assert ou[i][1] == ol[i][1] + 1 and ou[i][1] in (1025, 1409), f"{name}: the first differing outcome is {ou[i]} vs {ol[i]}: not the count edge"
    group = np.unique(ru["sel_docs"][0][i][1])
    assert len(group) == ou[i][1]
    return page2, i, ou[i], ol[i], group


def edge_masks(name, variant):
    """edge-low / edge-top / edge-elsewhere of an upper case: one doc disallowed each."""
    c = cases.get_case(name)
    mode = variant[0]
    page2, i, upper, lower, group = edge_site(name, variant)
    fd, fs, fc = full_ranking(c, mode)
    ranked = fd[0, :fc[0]].astype(np.int64) - c.doc_base
    top = ranked[1024:1024 + c.deep] if page2 else ranked[:c.k]  # the rows the step's page returns
    in_top = np.isin(group, top)
    assert in_top.any() and not in_top.all(), f"{name}: the group lies on one side of the top k"
    scoreless = np.setdiff1d(np.arange(c.n_docs), ranked)  # docs outside the group that no row can hold
    scoreless = np.setdiff1d(scoreless, group)
    beside = scoreless[np.isin(scoreless - 1, group)]  # the neighbouring bit of a group doc's, where there is one
    out = {}
    for key, doc in (("edge-low", group[~in_top][-1]), ("edge-top", group[in_top][0]), ("edge-elsewhere", (beside if len(beside) else scoreless)[0])):
        m = np.ones((1, c.n_docs), bool)
        m[0, doc] = False
        out[key] = (m, np.zeros(nq_of(c), np.int32))
    return out


_MASKS = {}


def masks_for(c, variant):
    """name -> (rows bool[n_rows, n_docs], q_filter or None) of every filtered run of the case.  Built from the case and the
    oracle's rows; `knock` sits in row 1 behind its complement, so a row addressed wrongly shows."""
    key = (c.name, variant[0], variant[1])
    if key not in _MASKS:
        n, nq = c.n_docs, nq_of(c)
        kn = knock_mask(c, variant[0])
        out = {"ones": (np.ones((1, n), bool), None),
               "knock": (np.stack([~kn, kn]), np.ones(nq, np.int32)),
               "none": (np.zeros((1, n), bool), None),
               "tail": (tail_mask(c)[None, :], None)}
        if c.name in _UPPER:
            out.update(edge_masks(_UPPER[c.name], variant))
        _MASKS[key] = out
    return _MASKS[key]


_UPPER = {}  # Case.name -> its CASES key, for the upper cases
for _name in PAIRS:
    _UPPER[cases.get_case(_name).name] = _name
DEEP_MASKS = ("ones", "knock", "edge-low", "edge-top", "edge-elsewhere")  # the masks that also run at top_k = 1024 + deep


def many_items(variant):
    """(q of 1 100 copies of the case's query, rows [knock, its complement], q_filter cycling (0, -1, 1), the three expected row
    sets by q_filter value, the plan)."""
    c = cases.get_case(MANY_CASE)
    assert nq_of(c) == 1
    terms, w = c.q[1].tolist(), c.q[2].tolist()
    q = _batch([(terms, w)] * MANY_ITEMS)
    kn = knock_mask(c, variant[0])
    rows = np.stack([kn, ~kn])
    q_filter = np.array([(0, -1, 1)[i % 3] for i in range(MANY_ITEMS)], np.int32)
    full = full_ranking(c, variant[0])
    exp = {r: filter_ref.filtered_rows(*full, [None if r < 0 else rows[r]], c.doc_base, c.k) for r in (0, -1, 1)}
    p = plan(c.n_tiles, c.tps, MANY_ITEMS, c.k, MANY_ITEMS)
    return q, rows, q_filter, exp, p


# ---- the tests -----------------------------------------------------------------------------------------------------------------
def _rows_equal(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(a, b))


_HITS = {}  # case -> {kind hit by a knock sensitivity check}, and the steps without a doc of T


def check_case(name):
    """Every condition of the case's masks, every variant; returns (kinds hit, steps whose range holds no result doc, tail is real)."""
    if name in _HITS:
        return _HITS[name]
    c = cases.get_case(name)
    hit, blind, tail_real = set(), [], False
    for vid, variant in case_variants(c):
        mode = variant[0]
        label = f"{name} {vid}"
        masks = masks_for(c, variant)
        ones_rows, _ = masks["ones"]
        # ones: the route of debug | 8 | 16, the oracle's rows
        r1 = masked_routes(c, variant, ones_rows, None)
        r0 = routes(c, variant, debug=c.debug | 8 | 16)
        assert r1["steps"] == r0["steps"] and r1["all_units"] == r0["all_units"] and all(r1["all_units"]), f"{label}: an all-ones row changes the route"
        assert all(t == 0 for t in r1["tau0"]) and all(t == 0 for t in r0["tau0"]), f"{label}: tau0 {r1['tau0']}"
        assert _rows_equal(expected(c, mode, ones_rows, None), cases.expected_rows(c, mode)), f"{label}: all-ones rows vs the oracle at k"
        assert not any(s[1] == "quads_unit" for st in r1["steps"] for s in st if len(s) > 1 and isinstance(s[1], str)), f"{label}: quads_unit in an all-tier-2 search"
        paths = [path_part(st) for st in r1["steps"]]
        # every mask: the path part is the all-ones route's
        for mname, (rows, qf) in masks.items():
            rm = masked_routes(c, variant, rows, qf)
            assert [path_part(st) for st in rm["steps"]] == paths, f"{label} {mname}: the dispatch consulted the mask"
            assert [x[0] for it in range(len(rm["steps"])) for x in rm["sel_docs"][it]] == [o for st in rm["steps"] for o in outcomes(st)], f"{label} {mname}"
        # knock: per serving step, an engine without the filter inside the step's range returns other rows
        rows, qf = masks["knock"]
        T = result_docs(c, mode)
        true_rows = expected(c, mode, rows, qf)
        assert not _rows_equal(true_rows, cases.expected_rows(c, mode)), f"{label}: knock takes nothing away"
        for st in r1["steps"]:
            for kind, lo, hi, what in serving_steps(c, st):
                if not np.any((T >= lo) & (T < hi)):
                    blind.append(f"{label}: {what}")
                    continue
                broken = rows.copy()
                broken[:, lo:hi] = True
                assert not _rows_equal(expected(c, mode, broken, qf), true_rows), f"{label}: {what} could ignore the filter unseen"
                hit.add(kind)
        # none: nothing anywhere
        rows, qf = masks["none"]
        ed, es, ec = expected(c, mode, rows, qf)
        assert np.all(ed == -1) and not es.view(np.uint32).any() and not ec.any()
        rn = masked_routes(c, variant, rows, qf)
        for st in rn["steps"]:
            assert all(o in (("fold_none", 0), ("early_return", 0), ("append_served", 0)) for o in outcomes(st)), f"{label} none: {outcomes(st)}"
            assert st[-1] == ("emit", 0, False) and not any(compacts(st)), f"{label} none: {st[-1]}"
        # tail: the ragged tile's docs of the ranking, without the last doc
        rows, qf = masks["tail"]
        ed, es, ec = expected(c, mode, rows, qf)
        G = 1 << c.tile_log2
        got = ed[ed >= 0].astype(np.int64) - c.doc_base
        assert np.all((got >= (c.n_tiles - 1) * G) & (got < c.n_docs - 1))
        tail_real = tail_real or len(got) > 0
        # edge: the three masks on the two sides of the comparison
        if name in PAIRS:
            page2, i, upper, lower, group = edge_site(name, variant)
            lo_case = cases.get_case(PAIRS[name])
            run = page2_routes if page2 else masked_routes
            lo_compact = compacts(run(lo_case, variant, np.ones((1, lo_case.n_docs), bool), None)["steps"][0])
            up_compact = compacts(run(c, variant, ones_rows, None)["steps"][0])
            for mname, want, want_compact in (("edge-low", lower, lo_compact), ("edge-top", lower, lo_compact), ("edge-elsewhere", upper, up_compact)):
                rows, qf = masks[mname]
                (st,) = run(c, variant, rows, qf)["steps"]
                assert outcomes(st)[i] == want, f"{label} {mname}: outcome {outcomes(st)[i]}, the pair's {'lower' if want == lower else 'upper'} side is {want}"
                assert compacts(st) == want_compact, f"{label} {mname}: compact {compacts(st)} vs {want_compact}"
                d = int(np.flatnonzero(~rows[0])[0])
                assert (d in group) == (mname != "edge-elsewhere")
    _HITS[name] = (hit, blind, tail_real)
    return _HITS[name]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_masks_of_a_case(name):
    hit, blind, _ = check_case(name)
    assert hit, f"{name}: no step of the route could be checked for sensitivity; steps without a result doc: {blind}"


def test_every_step_kind_is_hit():
    """Across the case list every kind of serving step a filtered search can take is hit by a knock sensitivity check.
    quads_unit is not among them: see the module docstring (asserted per case in check_case)."""
    hit, blind = set(), []
    for name in cases.CASES:
        h, b, _ = check_case(name)
        hit |= h
        blind += b
    assert hit == set(SERVING_KINDS), f"never hit: {sorted(set(SERVING_KINDS) - hit)}; steps whose range holds no result doc: {blind}"


def test_tail_is_a_real_comparison():
    """The ragged last tile returns rows under `tail` wherever it holds postings of the query: every D2 and D3 case and the D4
    cases at tl >= 13 (D4 at tl = 12 leaves its ragged tile empty: case_d4).  The other cases are named, not failed."""
    real = {name for name in cases.CASES if check_case(name)[2]}
    must = {n for n in cases.CASES if n.startswith(("D2-", "D3-", "D4-tl13", "D4-tl14"))}
    assert must and must <= real, f"`tail` returns nothing for {sorted(must - real)}; it returns rows for {sorted(real)}"
    print("tail returns no row for:", sorted(set(cases.CASES) - real))


def test_every_pair_has_its_masks():
    assert set(PAIRS) <= set(cases.CASES) and set(PAIRS.values()) <= set(cases.CASES)
    assert {n for n in cases.CASES if n.endswith(("-1025", "-1409", "-2433"))} == set(PAIRS)
    for name in PAIRS:
        c = cases.get_case(name)
        for vid, variant in case_variants(c):
            assert {"edge-low", "edge-top", "edge-elsewhere"} <= set(masks_for(c, variant)), f"{name} {vid}"
            page2, i, upper, lower, group = edge_site(name, variant)
            assert page2 == (name in PAGE2_PAIRS) and (c.deep > 0 or not page2)


def test_many_items_rows_differ_across_the_grid():
    c = cases.get_case(MANY_CASE)
    assert c.n_docs == 293
    r = routes(c, VARIANTS[0], allowed=[np.ones(c.n_docs, bool)])
    assert {s[1] for s in r["steps"][0] if len(s) > 1 and isinstance(s[1], str)} == {"flat"}, "the per-unit loop"
    for vid, variant in case_variants(c):
        q, rows, q_filter, exp, p = many_items(variant)
        assert p["items"] == MANY_ITEMS > T2_GRID_MAX and p["n_splits"] == 1 and len(q[0]) - 1 == MANY_ITEMS
        for a, b in ((0, -1), (0, 1), (-1, 1)):
            assert not _rows_equal(exp[a], exp[b]), f"{vid}: rows {a} and {b} give the same result"
        assert all(exp[r][2][0] > 0 for r in exp)
        for w in range(MANY_ITEMS - T2_GRID_MAX):  # a workgroup's second item: another row than its first
            assert w + T2_GRID_MAX < MANY_ITEMS and q_filter[w] != q_filter[w + T2_GRID_MAX]
        assert MANY_ITEMS - T2_GRID_MAX == 76
