"""Which units tier 1 serves and which it hands to tier 2, read out of the workspace after a search.

Every other sparse GPU test compares the final rows with the oracle; tier 2 rescans whatever tier 1 flags, so a tier-1
change that flags too much -- or everything -- still returns exact rows.  Here the caller-provided workspace (filled with
0xA5 before the search: tier 1 initialises its own slots, nothing may leak from a stale one) is decoded after the search
(tests/parity.py: search_ws, decode_routes) and compared with the restated hand-over rules (parity.tier1_routes) on the
directed corpora of tests/test_tier1_routes_cpu.py, which asserts on the CPU that each corpus reaches its edge:
  (a) the rows equal the oracle bit for bit;
  (b) every MUST_FLAG bit is set, every MUST_SERVE bit is clear (the directed cases state the whole set), and no bit is set
      outside the item's own unit range or at / beyond n_super;
  (c) the worklist is the items tier 1 cannot serve (nt > 64, k > 112) with nt > 0 plus the items with a set bit, each once;
  (d) with debug bit 8 every item with nt > 0 is on the worklist, no bit is set and the rows are still exact.
BM25 stores fp32 impacts, so fp16 values are run in dot mode only; the fp32 dot variant keeps the compact copy alone."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402  (checker only)
import test_tier1_routes_cpu as cases  # noqa: E402
from parity import decode_routes, item_queries, plan_workspace_bytes  # noqa: E402
from test_tier1_routes_cpu import VARIANTS  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()
    return sparse_rx


def _index(rx, c, variant):
    mode, vd, opts = variant
    return rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, c.idf, doc_lengths=c.doc_lengths, avgdl=c.avgdl, mode=mode, val_dtype=vd,
                                   tile_log2=c.tile_log2, unit_tiles=c.unit_tiles, doc_base=c.doc_base, **opts)


_ORACLE = {}


def _expected_rows(c, mode, k):
    """The oracle's rows of a case, computed once per (case, scoring, k) and shared; the given-order modes wherever a query
    lists its terms out of order or with a weight the default oracle skips."""
    key = (c.name, mode, k)
    if key not in _ORACLE:
        go = cases.given_order(c.q)
        if mode == "dot":
            m = oracle.MODE_TFIDF_F32_GIVEN_ORDER if go else oracle.MODE_TFIDF_F32
        else:
            m = oracle.MODE_BM25_F32_GIVEN_ORDER if go else oracle.MODE_BM25_F32
        ed, es, ec = oracle.search_batch(c.indptr, c.indices, c.data, c.doc_lengths, c.idf, *c.q, k, 1.2, 0.75, c.avgdl, mode=m)
        _ORACLE[key] = (np.where(ed >= 0, ed + c.doc_base, ed).astype(np.int32), es, ec)
    return _ORACLE[key]


def _assert_exact(got, exp, label):
    from test_gpu_parity import _assert_exact as check
    check(got, exp, label)


def _search(ix, c, k, target, debug):
    """One search with a workspace of the caller's, 0xA5 in every byte: (plan, rows, flag bits, worklist)."""
    import torch
    nq = len(c.q[0]) - 1
    ix.set_opts(target_blocks=target, debug=debug)
    p = cases.case_plan(c, k, target)
    assert plan_workspace_bytes(p, nq, k) == ix.workspace_bytes(nq, k), f"{c.name}: restated planner drifted from make_plan"
    ws = torch.full((ix.workspace_bytes(nq, k),), 0xA5, dtype=torch.uint8, device=ix.device)
    out = torch.full((nq, 2 * k + 1), -7, dtype=torch.int32, device=ix.device)
    dq = [torch.as_tensor(np.ascontiguousarray(x), device=ix.device) for x in c.q]
    ix.search_packed_device(*dq, k, out=out, workspace=ws)
    torch.cuda.synchronize()
    rows = out.cpu().numpy()
    bits, work, _ = decode_routes(ws.cpu().numpy(), p, nq, k)
    return p, (rows[:, :k].copy(), rows[:, k:2 * k].copy().view(np.float32), rows[:, 2 * k].copy()), bits, work


def check_routes(ix, c, variant, k=None, target=0, tier2_only=False, splits=None):
    """Assertions (a) - (c) of one search of case `c`, or (d) with tier2_only.  Returns (plan, routes, bits)."""
    k = c.k if k is None else k
    nq = len(c.q[0]) - 1
    label = f"{c.name} {variant[0]}-{variant[1]} k={k} target={target}" + (" debug 8" if tier2_only else "")
    p, got, bits, work = _search(ix, c, k, target, c.debug | (8 if tier2_only else 0))
    if splits is not None:
        assert (p["n_whole"], p["n_splits"]) == splits, f"{label}: plan {p['n_whole']} whole + x{p['n_splits']}, written for {splits}"
    _assert_exact(got, _expected_rows(c, variant[0], k), label)  # (a)
    r = cases.case_routes(c, p, variant, k=k)
    r["worklist"] = sorted(work)
    n_super = p["n_super"]
    assert len(work) == len(set(work)), f"{label}: an item twice on the worklist"
    if tier2_only:  # (d)
        assert not bits.any(), f"{label}: flag bits under debug 8"
        assert set(work) == set(np.flatnonzero(r["nt"] > 0).tolist()), f"{label}: worklist {sorted(work)}"
        return p, r, bits
    inside = np.zeros_like(bits)
    inside[:, :n_super] = r["in_range"]
    stray = np.argwhere(bits & ~inside)
    assert len(stray) == 0, f"{label}: bits outside the item's unit range (item, bit): {stray[:8].tolist()}"
    b = bits[:, :n_super]
    miss = np.argwhere(r["must_flag"] & ~b)
    assert len(miss) == 0, f"{label}: tier 1 served units it must flag (item, unit): {miss[:8].tolist()}"
    extra = np.argwhere(r["must_serve"] & b)
    assert len(extra) == 0, f"{label}: tier 1 flagged units it must serve (item, unit): {extra[:8].tolist()}"
    assert not b[r["all_t2"] | (r["nt"] == 0)].any(), f"{label}: flag bits of an item tier 1 does not serve"
    if c.flagged is not None:  # a directed case states the whole set, MAY units included
        exp = cases.expected_bits(c, p, r)
        assert np.array_equal(b, exp), f"{label}: flagged (item, unit) {np.argwhere(b).tolist()[:12]}, written for {np.argwhere(exp).tolist()[:12]}"
    on_list = (r["all_t2"] & (r["nt"] > 0)) | b.any(axis=1)
    assert set(work) == set(np.flatnonzero(on_list).tolist()), f"{label}: worklist {sorted(work)[:16]} vs {np.flatnonzero(on_list)[:16].tolist()}"  # (c)
    return p, r, bits


def _nq(c):
    return len(c.q[0]) - 1


@pytest.mark.parametrize("nt", cases.A_NTS)
def test_run_length_edges(rx, nt):
    """Case A: 4 LPT .. 12 LPT postings of one term are served (NR = 4 / 8 / 12 bodies), 12 LPT + 1 are flagged; whole queries
    (the units of a query pipelined through one wave) and one item per unit."""
    c = cases.case_a(nt)
    for variant in VARIANTS:
        ix = _index(rx, c, variant)
        for target in (_nq(c), 0):
            p, r, bits = check_routes(ix, c, variant, target=target, splits=(0, 1) if target else (0, 8))
            assert bits.sum() == _nq(c)
        check_routes(ix, c, variant, target=_nq(c), tier2_only=True)
        ix.close()


@pytest.mark.parametrize("kind", cases.B_KINDS)
def test_multi_term_resolutions(rx, kind):
    """Case B: 48 resolution visits are served, the 49th hands the unit over; term order ascending, descending, rotated."""
    c = cases.case_b(kind)
    for variant in VARIANTS:
        ix = _index(rx, c, variant)
        for target in (_nq(c), 0):
            p, r, bits = check_routes(ix, c, variant, target=target, splits=(0, 1) if target else (0, 5))
            assert bits.sum() == 3
        check_routes(ix, c, variant, target=_nq(c), tier2_only=True)
        ix.close()


def test_id_and_bitmap_edges(rx):
    """Case C: local ids 0, 31, 32, 16383, 16384, 49151, the sentinel words 1536, 1537, 1599, a ragged last unit, a doc_base."""
    c = cases.case_c()
    for variant in VARIANTS:
        ix = _index(rx, c, variant)
        assert ix.unit_tiles == 3 and ix.n_tiles == 7
        for target in (_nq(c), 0):
            p, r, bits = check_routes(ix, c, variant, target=target, splits=(0, 1) if target else (0, 3))
            assert not bits.any()
        check_routes(ix, c, variant, target=0, tier2_only=True)
        ix.close()


@pytest.mark.parametrize("first", [256, 257])
def test_full_list_on_the_first_unit(rx, first):
    """Case D: 256 entries fill the empty list exactly (served); the 257th finds it full with nothing to cut (flagged).  See
    case_d for the derivation from process()."""
    c = cases.case_d(first)
    for variant in VARIANTS:
        ix = _index(rx, c, variant)
        for target in (1, 0):
            p, r, bits = check_routes(ix, c, variant, target=target, splits=(0, 1) if target else (0, 3))
            assert r["may"].sum() == 1 and bits.sum() == (first > 256)
        check_routes(ix, c, variant, target=1, tier2_only=True)
        ix.close()


def test_full_list_redo_chain(rx):
    """Case D, the redo chain: 30 MUST_SERVE units, the list overflows every second unit, is cut to k = 112 and the unit redone."""
    c = cases.case_d_redo()
    for variant in VARIANTS:
        ix = _index(rx, c, variant)
        p, r, bits = check_routes(ix, c, variant, target=1, splits=(0, 1))
        assert r["must_serve"].sum() == 30 and not bits.any()
        p, r, bits = check_routes(ix, c, variant, target=3, splits=(0, 3))  # ten units per item: the chain inside every split
        assert not bits.any()
        ix.close()


@pytest.mark.parametrize("which", ["tail", "exact"])
def test_prologue_and_k(rx, which):
    """Case E: nt = 0 .. 65 in one batch (the scalar prologue's wide loads and its tail branch on the batch's last query, a
    negative weight), k on both sides of the bound columns' edges 1, 10, 100 and of tier 1's largest k."""
    c = cases.case_e(which)
    nq = _nq(c)
    for variant in VARIANTS:
        ix = _index(rx, c, variant)
        for k in cases.E_KS:
            for target in (16, 0):
                p, r, bits = check_routes(ix, c, variant, k=k, target=target)
                assert not r["may"].any()
                if k == 113:
                    assert r["all_t2"].all() and not bits.any()
        check_routes(ix, c, variant, k=112, target=16, tier2_only=True)
        ix.close()


F_CASES = [("A", 3), ("A", 8), ("A", 64), ("B", "two"), ("B", "eight"), ("B", "sixtyfour")]


@pytest.mark.parametrize("family,arg", F_CASES, ids=[f"{f}-{a}" for f, a in F_CASES])
def test_split_plans(rx, family, arg):
    """Case F: the corpora of A and B cut into 2, 3 and 4 doc-range splits per query and under a mixed plan (2 whole queries +
    1 x 2 splits).  A flag sits in the item whose range holds the unit, at the unit's global bit; the served 12 LPT / 48-visit
    unit and the flagged one next to it sit on either side of a split boundary or end a split."""
    c = cases.case_a(arg) if family == "A" else cases.case_b(arg)
    assert _nq(c) == 3
    fu = 5 if family == "A" else 2
    for variant in VARIANTS:
        ix = _index(rx, c, variant)
        for target, splits in zip(cases.F_TARGETS, ((0, 2), (0, 3), (0, 4), (2, 2))):
            p, r, bits = check_routes(ix, c, variant, target=target, splits=splits)
            q_of, split_of, nsq_of = item_queries(p, 3)
            items, units = np.nonzero(bits)
            assert units.tolist() == [fu] * 3 and sorted(q_of[items].tolist()) == [0, 1, 2]
            for it in items:  # the item whose [su_lo, su_hi) holds the unit
                lo = p["n_super"] * int(split_of[it]) // int(nsq_of[it])
                hi = p["n_super"] * (int(split_of[it]) + 1) // int(nsq_of[it])
                assert lo <= fu < hi
        check_routes(ix, c, variant, target=9, tier2_only=True)
        ix.close()


@pytest.mark.parametrize("name", list(cases.RANDOM))
def test_random_corpora(rx, name):
    """The random cases of the CPU file: everything served (an empty worklist), nearly everything flagged, and a mix."""
    c = cases.case_random(name)
    variant = VARIANTS[0]
    ix = _index(rx, c, variant)
    for target in (0, 64):
        p, r, bits = check_routes(ix, c, variant, target=target)
        b = bits[:, : p["n_super"]]
        if name == "served":
            assert not b.any() and r["worklist"] == []  # work[0] == 0
        else:
            assert b.sum() >= r["must_flag"].sum() > 0.2 * r["in_range"].sum()
    check_routes(ix, c, variant, target=0, tier2_only=True)
    ix.close()
