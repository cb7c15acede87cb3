"""The arithmetic of tests/sparse_scale.py with Python integers, and the generator against the real layout.

For every row of the table: each boundary it names is really crossed (planted blocks wholly below it, a run across it, planted
blocks wholly above it, in the units of the copy the boundary is named for); the device bytes stay under the cap; NO QUERY
TERM IS A FILLER TERM and the planted rows are well-formed -- the safety of the whole construction, since the kernels index
term_ptr / tile_skip / post with what the queries name; and the same generator, run with every boundary exponent lowered (the
only constant that changes), gives an index small enough to hold on the host whose every word of term_ptr, post, post16 and
tile_skip equals parity.np_build_blocks / np_compact_blocks of the same postings (filler postings included) and whose search
through the oracle gives the rows the big case expects."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import parity  # noqa: E402
import sparse_scale as T  # noqa: E402

IDS = [c.name for c in T.CASES]


def _blocks(lay):
    """[(first block, one past the last block)] of the planted terms that hold postings"""
    return [(p["ptr"] // 4, (p["ptr"] + p["extent"]) // 4) for p in lay.planted if p["extent"]]


def _unit_of_boundary(case, place):
    """(units per block, the boundary) so that block b lies below it iff (b + 1) * per <= B and at or above iff b * per >= B"""
    if place[0] == "bytes":
        return 4 * case.words(place[1]), 1 << place[2]
    if place[0] == "words":
        return case.words(place[1]), 1 << place[2]
    return 4, 1 << place[1]


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_case_crosses_its_boundaries(case):
    lay = T.build(case)
    named = [pl for pl in lay.places if pl is not None]
    assert named or case.vocab_rule, f"{case.name}: written for nothing"
    for pl in named:
        if "block" in pl:
            per, B = _unit_of_boundary(case, pl["place"])
            assert pl["place"][0] == "pos" or pl["place"][1] in case.copies, "a boundary of a copy the case does not carry"
            bB = pl["block"]
            assert bB * per <= B < (bB + 1) * per or bB * per == B
            assert any(hi * per <= B for lo, hi in _blocks(lay)), f"{case.name} {pl['place']}: no planted term ends at or below it"
            assert any(lo * per >= B for lo, hi in _blocks(lay)), f"{case.name} {pl['place']}: no planted term starts at or above it"
            p = lay.planted[pl["small"]]
            sk = lay.skip_row(pl["small"])
            lo = (p["ptr"] + int(sk[pl["unit"] * case.unit_tiles])) // 4
            hi = (p["ptr"] + int(sk[min((pl["unit"] + 1) * case.unit_tiles, case.n_tiles)])) // 4
            assert lo < bB < hi and hi - lo == pl["run_blocks"], f"{case.name} {pl['place']}: the run [{lo}, {hi}) does not straddle block {bB}"
            assert lo * per < B and hi * per > B  # ... and the posting array goes on well past it
            assert (lay.n_blocks + T.BLOCK_PAD) * per > B
        else:
            e = pl["entry"]
            t = lay.planted[pl["small"]]["term"]
            assert t * case.row <= e < (t + 1) * case.row and e == 1 << 31
            terms = [p["term"] for p in lay.planted]
            assert any((x + 1) * case.row <= e for x in terms) and any(x * case.row >= e for x in terms)
            assert lay.vocab * case.row > 1 << 31 and lay.vocab * case.row * 4 > 8 << 30
    if "pos" in [pl["place"][0] for pl in named]:
        assert int(lay.term_ptr[-1]) >= 1 << 31
    # term 0 and the last term before the sentinel pad are planted, and both are queried
    assert lay.planted[0]["term"] == 0 and lay.planted[0]["ptr"] == 0
    last = lay.planted[-1]
    assert last["term"] == lay.vocab - 1 and last["ptr"] + last["extent"] == 4 * lay.n_blocks
    assert {0, lay.vocab - 1} <= set(lay.queries[1].tolist())
    assert case.doc_base_top >= 0 and case.doc_base_top + case.n_docs == (1 << 31) - 2


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_device_bytes_under_the_cap(case):
    lay = T.build(case)
    assert lay.device_bytes() <= T.CAP_BYTES and T.arena_bytes() <= T.CAP_BYTES
    for copy in case.copies:
        assert lay.posting_bytes(copy) == (lay.n_blocks + 256) * T.BLOCK_WORDS[(case.val, copy)] * 4
    for what, nbytes in T.OUT_OF_REACH.items():
        assert nbytes >= T.CAP_BYTES, what


def test_skip_table_cases_sit_on_the_clause():
    by = {c.name: T.build(c) for c in T.CASES}
    lt, ge, gt = by["s-lt30"], by["s-ge30"], by["s-gt31"]
    row = lt.case.row
    assert row == 1025 and lt.case.n_tiles == 1024 and lt.case.tile_log2 == 6
    assert lt.vocab * row < 1 << 30 <= (lt.vocab + 1) * row          # the largest product below 2^30
    assert (ge.vocab - 1) * row < 1 << 30 <= ge.vocab * row          # the first at or above it
    assert ge.vocab == lt.vocab + 1
    assert 0 < (1 << 32) - 4 * lt.vocab * row <= 8192                 # the last row ends a few KB under byte 2^32 of the table
    assert lt.planted[-1]["term"] == lt.vocab - 1 and lt.planted[-1]["extent"] > 0
    assert T.tier1_serves(lt) and not T.tier1_serves(ge) and not T.tier1_serves(gt)
    for lay in (lt, ge, gt):
        for nt in (1, 4, 64):
            assert parity.tier1_cannot_serve(nt, T.K, 64, 6, lay.vocab, 1024, 0) == (lay is not lt)
    assert gt.vocab * row > 1 << 31
    for c in T.CASES:
        if c.name.startswith("p-"):
            assert T.tier1_serves(T.build(c)) == ("post16" in c.copies), c.name


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_no_query_term_is_a_filler_term(case):
    lay = T.build(case)
    q_ptr, q_term, q_w = lay.queries
    planted = {p["term"]: p for p in lay.planted}
    assert len(planted) == len(lay.planted)
    assert q_ptr[0] == 0 and np.all(np.diff(q_ptr) > 0) and q_ptr[-1] == len(q_term) == len(q_w)
    for q in range(len(q_ptr) - 1):
        ts = q_term[q_ptr[q]:q_ptr[q + 1]].tolist()
        assert len(set(ts)) == len(ts), f"{case.name}: query {q} repeats a term"
        assert all(t in planted and 0 <= t < lay.vocab for t in ts), f"{case.name}: query {q} names a filler term"
    assert set(q_term.tolist()) == set(planted), "every planted term is queried"
    G = 1 << case.tile_log2
    assert case.n_tiles == -(-case.n_docs // G) and case.unit_tiles * G == T.U
    assert "post16" not in case.copies or case.unit_tiles * G <= 49152
    tp = lay.term_ptr
    assert len(tp) == lay.vocab + 1 and tp[0] == 0 and np.all(np.diff(tp) >= 0) and np.all(tp % 4 == 0) and int(tp[-1]) == 4 * lay.n_blocks
    for p in lay.planted:
        sk = lay.skip_row(p["small"]).astype(np.int64)
        assert len(sk) == case.row and sk[0] == 0 and np.all(np.diff(sk) >= 0), f"{case.name}: skip row of term {p['term']}"
        assert int(tp[p["term"]]) == p["ptr"] and int(tp[p["term"] + 1]) == p["ptr"] + p["extent"] and sk[-1] == p["extent"]
        assert p["ptr"] + int(sk[case.n_tiles]) <= 4 * lay.n_blocks
        assert np.all(sk[::case.unit_tiles] % 4 == 0) and sk[-1] % 4 == 0
        # the blocks hold this term's docs in ascending order inside every unit's run, sentinels of THIS term behind them
        b = lay.blocks_of(p["small"])
        d = b[:, :4].reshape(-1).astype(np.int64)
        assert len(d) == p["extent"] and np.all((d >= 0) | (d == -1 - 32 * (p["term"] % 64))) and d.max(initial=-1) < case.n_docs
    pad = lay.pad_blocks()
    j = np.arange(T.BLOCK_PAD)
    assert pad.shape == (T.BLOCK_PAD, case.words("post")) and np.array_equal(pad[:, :4], np.repeat(-1 - 32 * (j % 64), 4).reshape(-1, 4))
    assert not pad[:, 4:].any()
    # planted extents do not overlap, and every filler extent could really be filled
    spans = sorted((p["ptr"], p["ptr"] + p["extent"]) for p in lay.planted)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    cap = case.filler_cap()
    for g in lay.gaps:
        assert np.all(g["extents"] >= 0) and np.all(g["extents"] <= cap) and np.all(g["extents"] % 4 == 0)


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_planted_paths(case):
    """the restated hand-over rules on the planted postings: the runs of 4, 8, 12 LPT and the 48-visit unit are tier 1's, the
    runs of 12 LPT + 1, the 49-visit unit and the long runs of H are handed over, nothing is left to the list's state; tier 2
    then takes the hash unit for H's unit 5 and the wave-level dense path for its unit 6"""
    lay = T.build(case)
    nq = len(lay.queries[0]) - 1
    kinds = [g[0] for g in case.groups]
    assert {"A", "B", "H", "E"} == set(kinds)
    doc_len = np.ones(case.n_docs, np.float32)
    for target in (nq, 0):
        p = parity.plan(case.n_tiles, case.unit_tiles, nq, T.K, target)
        assert p["n_super"] == case.n_units
        r = parity.tier1_routes(*lay.csr, doc_len, lay.idf_small, lay.queries_small, case.tile_log2, case.unit_tiles, T.K, p, term_bound=True,
                                mode="dot", val_dtype=case.val)
        assert not r["may"].any() and not r["all_t2"].any(), f"{case.name}: a unit is left to the state of tier 1's list"
        q_of, _, _ = parity.item_queries(p, nq)
        flagged = {(int(q_of[i]), int(u)) for i, u in np.argwhere(r["must_flag"])}
        exp, q = set(), 0
        for kind in kinds:
            if kind == "A":
                exp.add((q, 5))
            elif kind == "B":
                exp |= {(q, 2), (q + 1, 2)}
            elif kind == "H":
                exp |= {(q, 5), (q, 6)}
            q += len(T.GROUPS[kind](0, case.n_docs)[2])
        assert q == nq and flagged == exp, f"{case.name}: flagged {sorted(flagged)}, written for {sorted(exp)}"
    t2 = parity.tier2_routes(*lay.csr, doc_len, lay.idf_small, lay.queries_small, case.tile_log2, case.unit_tiles, T.K, p, 0, r["must_flag"],
                             mode="dot", val_dtype=case.val, layout=(lay.small[0], _as_f32_blocks(lay), lay.small[2].reshape(-1), lay.small[3]))
    steps = [s for item in t2["steps"] for s in item if isinstance(s[0], (int, np.integer))]
    assert {s[1] for s in steps} == {"hash", "quads_unit"}, {s[1] for s in steps}
    assert sum(s[1] == "quads_unit" for s in steps) == kinds.count("H") and all(s[2] == 4096 for s in steps if s[0] == 5 and s[1] == "hash" and s[2] > 1000)


def _as_f32_blocks(lay):
    """tier2_routes reads doc ids out of 8-word blocks: the planted docs with zero values"""
    post = lay.small[1]
    out = np.zeros((len(post), 8), np.int32)
    out[:, :4] = post[:, :4]
    return out.reshape(-1)


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_generator_is_the_real_layout(case):
    """the scaled-down build: every word against np_build_blocks / np_compact_blocks of the same postings, filler included"""
    lay = T.build(case, case.shrink)
    big = T.build(case)
    assert [pl and pl["place"] for pl in lay.places] == [pl and pl["place"] for pl in big.places]
    for pl in lay.places:
        if pl and "block" in pl:  # the same boundary, 2^shrink times nearer
            assert pl["block"] == case.boundary_block(pl["place"], case.shrink) > 0
    n_fill = sum(int((g["extents"] > 0).sum()) for g in lay.gaps)
    assert (n_fill > 0) == case.name.startswith("p-") and lay.vocab > len(lay.planted)
    dt = T.VAL_DTYPE[case.val]
    csr = T.full_csr(lay)
    tp, post, skip, nb = parity.np_build_blocks(*csr, case.n_docs, lay.vocab, case.tile_log2, case.unit_tiles, dt, T.BLOCK_PAD)
    got_post, got_skip, idf = T.materialize(lay)
    assert nb == lay.n_blocks and np.array_equal(tp, lay.term_ptr)
    assert np.array_equal(post, got_post.reshape(-1)), "post"
    assert np.array_equal(skip, got_skip.reshape(-1)), "tile_skip"
    if "post16" in case.copies:
        exp16 = parity.np_compact_blocks(post, T.U, dt).reshape(nb + T.BLOCK_PAD, -1)
        for p in lay.planted:
            assert np.array_equal(exp16[p["ptr"] // 4: (p["ptr"] + p["extent"]) // 4], lay.blocks_of(p["small"], "post16")), p
        assert np.array_equal(exp16[nb:], lay.pad_blocks("post16"))
        assert np.array_equal(exp16, parity.np_compact_blocks(got_post.reshape(-1), T.U, dt).reshape(nb + T.BLOCK_PAD, -1))
    # the same planted data as the big case, and the same rows through the oracle on the WHOLE small index with the real ids
    assert all(np.array_equal(a, b) for a, b in zip(lay.csr, big.csr)) and np.array_equal(lay.queries_small[1], big.queries_small[1])
    assert np.array_equal(lay.small[2], big.small[2])
    full_small = T.full_scores(csr, idf, lay.queries, case.n_docs)
    full_big = T.full_scores(big.csr, big.idf_small, big.queries_small, case.n_docs)
    assert np.array_equal(full_small.view(np.uint32), full_big.view(np.uint32))
    rows = T.ranked_rows(full_big, T.K, case.doc_base_top)
    assert all(np.array_equal(a, b) for a, b in zip(rows, T.ranked_rows(full_small, T.K, case.doc_base_top)))
    assert rows[2].min() >= 1 and rows[0].max() == (1 << 31) - 3, "every query has results; the last doc of the shard is one"
    import oracle
    od, os_, oc = oracle.search_batch(*csr, None, idf, *lay.queries, T.K, mode=oracle.MODE_TFIDF_F32_GIVEN_ORDER)
    assert np.array_equal(oc, rows[2]) and np.array_equal(os_.view(np.uint32), rows[1].view(np.uint32))
    assert np.array_equal(np.where(od >= 0, od + case.doc_base_top, -1), rows[0])


def test_workspace_case_is_the_smallest_batch_past_byte_2_32():
    nq = T.ws_nq()
    first = T.ws_first_start_past(nq)
    assert first is not None and all(T.ws_first_start_past(n) is None for n in range(nq - 4000, nq))
    p = T.ws_plan(nq)
    assert p["n_splits"] == 2 and p["lists_per_q"] == 4 and p["t2_everything"] and p["merge_kernel"] == "block"
    assert p["n_whole"] > 0 and p["tail"] > 0, "whole queries and split ones in one batch"
    w = parity.search_ws(p, nq, T.WS_K)
    print(f"nq = {nq}: {first} starts at byte {w[first]}, the workspace ends at {w['end'] + 256}")
    assert w["cand_score"] < 1 << 31 < w["cand_count"] < 1 << 32 < w[first], "the score lists lie across byte 2^31, the counts end past 2^32"
    assert parity.plan_workspace_bytes(p, nq, T.WS_K) == w["end"] + 256 > 1 << 32
    assert T.ws_device_bytes() <= T.CAP_BYTES and T.ws_device_bytes() <= T.arena_bytes() and T.ws_device_bytes(nq) < T.ws_device_bytes()
    p2 = T.ws_plan(T.WS_NQ2)
    w2 = parity.search_ws(p2, T.WS_NQ2, T.WS_K)
    assert p2["n_splits"] == 2 and p2["n_whole"] > 0 and 1 << 32 < w2["cand_score"] < (1 << 32) + (1 << 20)
    assert parity.search_ws(T.ws_plan(T.WS_NQ2 - 1), T.WS_NQ2 - 1, T.WS_K)["cand_score"] == 1 << 32
