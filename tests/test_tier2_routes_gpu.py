"""The directed tier-2 cases of tests/test_tier2_routes_cpu.py on the MI355X, bit for bit against the oracle.

Which of tier 2's paths serves a unit cannot be seen from outside the kernel; the CPU file asserts through the restated
dispatch (parity.tier2_routes) that every case sits on the comparison it was written for, and this file runs each case
  (a) with a workspace of the caller's filled with 0xA5 and `out` filled with -7, through search_packed_device, rows equal to
      the oracle's bit for bit, under every variant the case's search allows (BM25 stores fp32; fp16 values in dot mode; the
      fp32 dot variant keeps the compact copy alone and is left out where the search uses another unit than the built one);
  (b) with the plan pinned: plan_workspace_bytes(...) == ix.workspace_bytes(...);
  (c) with the flag bits tier 1 left decoded from the workspace (decode_routes) and fed to tier2_routes: the route is the one
      the case states -- a tier-1 change that stops flagging a unit fails the case instead of letting it test nothing;
  (d) where tier 1 serves nothing (debug 8, k > 112, nt > 64, another unit), the worklist holds every item with nt > 0;
  (e) cases with `deep` also at top_k = 1024 + r: the second page is a search-after (the AFTER instances).  For S1-2432 /
      S1-2433 the CPU file asserts through the restatement's bound that this page sees 1 408 / 1 409 candidates in its first
      tile group and that the bound's doc lies inside it (test_search_after_bound_lands_on_the_edge); for the other deep
      cases the page only has to return the oracle's rows."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_tier2_routes_cpu as cases  # noqa: E402
from parity import decode_routes, plan_workspace_bytes  # noqa: E402
from test_tier1_routes_cpu import VARIANTS, VARIANT_IDS  # noqa: E402

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


def _run(rx, c, variant):
    import torch
    mode, vd, opts = variant
    label = f"{c.name} {mode}-{vd}"
    ix = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, c.idf, doc_lengths=c.doc_lengths, avgdl=c.avgdl, mode=mode, val_dtype=vd,
                                 tile_log2=c.tile_log2, unit_tiles=c.unit_tiles, doc_base=c.doc_base, **opts)
    try:
        assert ix.unit_tiles == c.unit_tiles and ix.n_tiles == c.n_tiles
        nq, k = len(c.q[0]) - 1, c.k
        ix.set_opts(supertile_log2=c.sl, unit_tiles=c.override, target_blocks=c.target, debug=c.debug)
        p = cases.case_plan(c)
        assert plan_workspace_bytes(p, nq, k) == ix.workspace_bytes(nq, k), f"{label}: restated planner drifted from make_plan"  # (b)
        ws = torch.full((ix.workspace_bytes(nq, k),), 0xA5, dtype=torch.uint8, device=ix.device)
        out = torch.full((nq, 2 * k + 1), -7, dtype=torch.int32, device=ix.device)
        dq = [torch.as_tensor(np.ascontiguousarray(x), device=ix.device) for x in c.q]
        ix.search_packed_device(*dq, k, out=out, workspace=ws)
        torch.cuda.synchronize()
        rows = out.cpu().numpy()
        got = (rows[:, :k].copy(), rows[:, k:2 * k].copy().view(np.float32), rows[:, 2 * k].copy())
        _assert_exact(got, cases.expected_rows(c, mode), label)  # (a)
        bits, work, _ = decode_routes(ws.cpu().numpy(), p, nq, k)
        r = cases.case_routes(c, variant, flags=bits)
        c.expect(r, c)  # (c)
        assert len(work) == len(set(work))
        opened = {i for i, steps in enumerate(r["steps"]) if steps[0] != ("skip",)}
        assert set(work) == opened, f"{label}: worklist {sorted(work)} vs the items with work {sorted(opened)}"
        if all(r["all_units"]):  # (d)
            nts = np.diff(c.q[0])
            assert not bits.any() and len(work) == p["items"] and np.all(nts > 0), f"{label}: worklist {sorted(work)}"
        if c.deep:  # (e)
            kd = 1024 + c.deep
            _assert_exact(ix.search(*c.q, kd), cases.expected_rows(c, mode, kd), f"{label} top_k={kd}")
    finally:
        ix.close()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case(rx, name):
    c = cases.get_case(name)
    for vi in c.variants:
        _run(rx, c, VARIANTS[vi])


def test_search_after_page_inside_a_tie_group(rx):
    """S6: the tie case of S3 paged by hand under the general selection, every variant: page 2 starts after the 60th row, inside
    the group of 1 200 docs scoring 2 that straddles the list and the second tile group."""
    import torch
    c = cases.get_case("S3-ties")
    for vi in c.variants:
        mode, vd, opts = VARIANTS[vi]
        ix = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, c.idf, doc_lengths=c.doc_lengths, avgdl=c.avgdl, mode=mode, val_dtype=vd,
                                     tile_log2=c.tile_log2, unit_tiles=1, **opts)
        try:
            ix.set_opts(debug=c.debug)
            ed, es, ec = cases.expected_rows(c, mode)
            assert es[0, 59] == es[0, 60] == es[0, 699]  # the bound and both ends of the page lie inside the tie group
            dq = [torch.as_tensor(np.ascontiguousarray(x), device=ix.device) for x in c.q]
            after = (torch.as_tensor(ed[:, 59].copy(), device=ix.device), torch.as_tensor(es[:, 59].copy(), device=ix.device))
            d, s, n = ix.search_device(*dq, 640, after=after)
            torch.cuda.synchronize()
            label = f"tie page {VARIANT_IDS[vi]}"
            assert int(n[0]) == 640, label
            assert np.array_equal(d.cpu().numpy()[0], ed[0, 60:700]) and np.array_equal(s.cpu().numpy()[0].view(np.uint32), es[0, 60:700].view(np.uint32)), label
        finally:
            ix.close()
