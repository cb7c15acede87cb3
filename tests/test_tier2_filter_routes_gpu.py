"""The directed tier-2 cases under doc filters on the MI355X: the filtered instances of csrc/tier2_filter.hip, bit for bit.

tests/test_tier2_filter_routes_cpu.py builds the masks of every case (masks_for) and asserts without a GPU that they mean
something: per step of the route an engine that lost the filter there would return other rows (`knock`), one filter bit moves
a selection across its count edge (`edge-*`), and the dispatch never reads the mask.  This file runs them.  Per (case,
variant) -- the case's VARIANTS plus the fp16 compact-only form, the <__half, compact> instance -- the index is built once, and
for every mask
  (a) search_packed_device with the caller's workspace filled with 0xA5 and `out` with -7 returns filter_ref.filtered_rows of
      the oracle's unfiltered ranking at k = n_docs, bit for bit: ids, score bits, counts, padding (`knock` also through
      search_device);
  (b) the plan is the restated one (workspace bytes), the worklist decoded from the workspace holds every item once and no
      flag bit is set: a filtered search leaves nothing to tier 1;
  (c) cases with `deep` run `ones`, `knock` and the edge masks also at top_k = 1024 + r through search(): page 2 is a
      search-after under the filter (for S1-2433 the edge masks sit on that page's selection).
many_items: 1 100 one-item queries whose filter rows cycle (0, -1, 1), more items than tier 2's grid of 1 024, so 76
workgroups serve a second item that carries another row than their first."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_tier2_filter_routes_cpu as fcases  # noqa: E402
import test_tier2_routes_cpu as cases  # noqa: E402
from parity import decode_routes, plan_workspace_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()
    return sparse_rx


def _assert_exact(got, exp, label):
    from test_gpu_parity import _assert_exact as check
    check(got, exp, label)


def _build(rx, c, variant):
    mode, vd, opts = variant
    ix = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, c.idf, doc_lengths=c.doc_lengths, avgdl=c.avgdl, mode=mode, val_dtype=vd,
                                 tile_log2=c.tile_log2, unit_tiles=c.unit_tiles, doc_base=c.doc_base, **opts)
    assert ix.unit_tiles == c.unit_tiles and ix.n_tiles == c.n_tiles
    return ix


def _packed(ix, dq, nq, k, flt, qf, ws):
    """One filtered search_packed_device into a poisoned workspace and output; (host triple, workspace bytes on the host)."""
    import torch
    ws.fill_(0xA5)
    out = torch.full((nq, 2 * k + 1), -7, dtype=torch.int32, device=ix.device)
    ix.search_packed_device(*dq, k, out=out, workspace=ws, filter=flt, q_filter=qf)
    torch.cuda.synchronize()
    rows = out.cpu().numpy()
    return (rows[:, :k].copy(), rows[:, k:2 * k].copy().view(np.float32), rows[:, 2 * k].copy()), ws.cpu().numpy()


def _run(rx, c, vid, variant):
    import torch
    mode = variant[0]
    nq, k = fcases.nq_of(c), c.k
    masks = fcases.masks_for(c, variant)
    ix = _build(rx, c, variant)
    try:
        ix.set_opts(supertile_log2=c.sl, unit_tiles=c.override, target_blocks=c.target, debug=c.debug)
        p = cases.case_plan(c)
        assert plan_workspace_bytes(p, nq, k) == ix.workspace_bytes(nq, k), f"{c.name} {vid}: restated planner drifted from make_plan"
        ws = torch.empty((ix.workspace_bytes(nq, k),), dtype=torch.uint8, device=ix.device)
        dq = [torch.as_tensor(np.ascontiguousarray(x), device=ix.device) for x in c.q]
        assert np.all(np.diff(c.q[0]) > 0)
        for mname, (rows, q_filter) in masks.items():
            label = f"{c.name} {vid} {mname}"
            flt = rx.DocFilter.from_masks(rows, device=ix.device, doc_base=c.doc_base)
            qf = None if q_filter is None else torch.as_tensor(np.asarray(q_filter, np.int32), device=ix.device)
            exp = fcases.expected(c, mode, rows, q_filter)
            got, ws_host = _packed(ix, dq, nq, k, flt, qf, ws)
            _assert_exact(got, exp, label)
            bits, work, _ = decode_routes(ws_host, p, nq, k)
            assert not bits.any(), f"{label}: a flag bit in a filtered search"
            assert sorted(work) == list(range(p["items"])), f"{label}: worklist {sorted(work)}"
            if mname == "knock":
                d, s, n = ix.search_device(*dq, k, filter=flt, q_filter=qf)
                torch.cuda.synchronize()
                _assert_exact((d.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()), exp, f"{label} search_device")
            if c.deep and mname in fcases.DEEP_MASKS:
                kd = 1024 + c.deep
                _assert_exact(ix.search(*c.q, kd, filter=flt, q_filter=q_filter), fcases.expected(c, mode, rows, q_filter, k=kd), f"{label} top_k={kd}")
    finally:
        ix.close()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case(rx, name):
    c = cases.get_case(name)
    for vid, variant in fcases.case_variants(c):
        _run(rx, c, vid, variant)


def test_many_items(rx):
    """More work items than workgroups: the second item of a workgroup republishes the filter row (another row set, or none).
    The second run follows a filtered search that left the worklist non-empty (the first): its grid is the full one too."""
    import torch
    c = cases.get_case(fcases.MANY_CASE)
    for vid, variant in fcases.case_variants(c):
        q, rows, q_filter, exp, p = fcases.many_items(variant)
        nq, k = fcases.MANY_ITEMS, c.k
        ix = _build(rx, c, variant)
        try:
            ix.set_opts(target_blocks=nq, debug=c.debug)
            assert plan_workspace_bytes(p, nq, k) == ix.workspace_bytes(nq, k)
            ws = torch.empty((ix.workspace_bytes(nq, k),), dtype=torch.uint8, device=ix.device)
            dq = [torch.as_tensor(np.ascontiguousarray(x), device=ix.device) for x in q]
            flt = rx.DocFilter.from_masks(rows, device=ix.device, doc_base=c.doc_base)
            qf = torch.as_tensor(q_filter, device=ix.device)
            want = tuple(np.concatenate([exp[int(r)][j] for r in q_filter]) for j in range(3))
            for run in (1, 2):
                got, ws_host = _packed(ix, dq, nq, k, flt, qf, ws)
                _assert_exact(got, want, f"many_items {vid} run {run}")
                bits, work, _ = decode_routes(ws_host, p, nq, k)
                assert not bits.any() and sorted(work) == list(range(nq)), f"many_items {vid} run {run}: worklist of {len(work)}"
        finally:
            ix.close()
