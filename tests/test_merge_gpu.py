"""The public top-k merge entry points against the NumPy restatement (tests/merge_ref.py), bit for bit.

srx_merge_topk (plain and gathered layouts), srx_merge_topk_packed and srx_merge_topk_packed_out are called through the C
ABI with the test's own buffers: every output word is pre-filled with a poison word and sits between two guard rows, so a
row the kernels skip, a word they leave out and a write outside the rows all show.  Every case names the kernels it is
written for (wave / block / tree levels, merge_ref.dispatch, pinned to the library in test_merge_cpu.py) and runs every
input family through all four layouts from the same logical input.  The merge does no arithmetic: there is no tolerance.

Safety: every read of the kernels is bounded by r < k and l < n_lists inside buffers sized [nq][n_lists][k] here, whatever
the counts say, and every write lands in rows of the sizes allocated below; nothing is retried."""
import numpy as np
import pytest

from merge_ref import (BIG_CASES, BIG_FAMILIES, CASES, POISON, bucket, case_families, case_seed, dispatch, make_input, merge,
                       packed_rows, tie_boundary_ok, to_gathered, to_packed, to_plain)

pytestmark = pytest.mark.gpu

LAYOUTS = ("plain", "gathered", "packed", "packed_out")
GUARD_WORDS = 64  # poisoned words behind the workspace


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from sparse_rx import _capi
    return torch, _capi.lib(), torch.device("cuda", 0)


def _words(a):
    """Any 4-byte array as int32 words (scores as their bit patterns)."""
    return np.ascontiguousarray(a).view(np.int32)


class _Guarded:
    """`rows` rows of `width` int32 words with one guard row before and one after, every word poisoned."""

    def __init__(self, torch, dev, rows, width):
        self.t = torch.full((rows + 2, width), POISON, dtype=torch.int32, device=dev)
        self.ptr = self.t[1:].data_ptr()

    def read(self, what):
        host = self.t.cpu().numpy()
        assert (host[0] == POISON).all() and (host[-1] == POISON).all(), f"{what}: a guard row was written"
        return host[1:-1]


def _same(got, exp, what):
    got, exp = _words(got), _words(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        i = tuple(int(x) for x in bad[0])
        poisoned = int((got == POISON).sum() - (exp == POISON).sum())
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {i}: got {int(got[i]) & 0xFFFFFFFF:#010x}, "
                             f"expected {int(exp[i]) & 0xFFFFFFFF:#010x}; {poisoned} words still hold the poison")


def _upload(torch, dev, a):
    return torch.from_numpy(_words(a)).to(dev)


def _run_layout(gpu, layout, lists, k, label, stream=None):
    """One entry point on one layout of `lists`; returns the result as packed rows [nq][2k+1] (int32 words)."""
    torch, L, dev = gpu
    nq, n_lists, _ = lists[0].shape
    need = dispatch(n_lists, k, nq).workspace_bytes
    assert need % 4 == 0
    ws = torch.full((need // 4 + GUARD_WORDS,), POISON, dtype=torch.int32, device=dev)
    ws_ptr = ws.data_ptr() if need else None  # no tree: the header allows NULL
    sp = (stream or torch.cuda.current_stream(dev)).cuda_stream
    if layout in ("plain", "gathered"):
        d, s, c = (_upload(torch, dev, a) for a in (to_plain(lists) if layout == "plain" else to_gathered(lists)))
        od, os_, oc = _Guarded(torch, dev, nq, k), _Guarded(torch, dev, nq, k), _Guarded(torch, dev, nq, 1)
        rc = L.srx_merge_topk(0, d.data_ptr(), s.data_ptr(), c.data_ptr(), nq, n_lists, k, int(layout == "gathered"), od.ptr, os_.ptr,
                              oc.ptr, ws_ptr, need, sp)
    else:
        p = _upload(torch, dev, to_packed(lists))
        if layout == "packed":
            od, os_, oc = _Guarded(torch, dev, nq, k), _Guarded(torch, dev, nq, k), _Guarded(torch, dev, nq, 1)
            rc = L.srx_merge_topk_packed(0, p.data_ptr(), nq, n_lists, k, od.ptr, os_.ptr, oc.ptr, ws_ptr, need, sp)
        else:
            op = _Guarded(torch, dev, nq, 2 * k + 1)
            rc = L.srx_merge_topk_packed_out(0, p.data_ptr(), nq, n_lists, k, op.ptr, ws_ptr, need, sp)
    assert rc == 0, (label, layout, rc, L.srx_last_error())
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    what = f"{label} [{layout}]"
    assert (ws[need // 4:].cpu().numpy() == POISON).all(), f"{what}: written behind the workspace"
    if layout == "packed_out":
        return op.read(what)
    return np.concatenate([od.read(what + " docs"), os_.read(what + " scores"), oc.read(what + " counts")], axis=1)


def _check_case(gpu, n_lists, k, want, nq, family, stream=None):
    assert bucket(n_lists, k) == want, "the row belongs to another bucket: move the row"
    label = f"{n_lists}x{k} nq={nq} {want} {family}"
    lists = make_input(family, nq, n_lists, k, case_seed(n_lists, k, nq, family))
    if family == "ties":
        ok = tie_boundary_ok(lists, k, dispatch(n_lists, k).fan)
        assert ok.all(), f"{label}: the k-th boundary is not inside a tie group across lists in queries {np.flatnonzero(~ok)} (pick another seed)"
    exp = packed_rows(merge(lists, k))
    for layout in LAYOUTS:
        got = _run_layout(gpu, layout, lists, k, label, stream)
        _same(got[:, 2 * k], exp[:, 2 * k], f"{label} [{layout}] counts")
        _same(got[:, :k], exp[:, :k], f"{label} [{layout}] docs")
        _same(got[:, k:2 * k], exp[:, k:2 * k], f"{label} [{layout}] score bits")


_PARAMS = [(c, f) for c in CASES for f in case_families(c[0])]
_BIG = [(c, f) for c in BIG_CASES for f in case_families(c[0], BIG_FAMILIES)]


def _id(p):
    (n_lists, k, want, nq), family = p
    return f"{n_lists}x{k}-nq{nq}-{want}-{family}"


@pytest.mark.parametrize("case,family", _PARAMS, ids=[_id(p) for p in _PARAMS])
def test_merge_entry_points(gpu, case, family):
    _check_case(gpu, *case, family)


@pytest.mark.parametrize("case,family", _BIG, ids=[_id(p) for p in _BIG])
def test_merge_entry_points_nq1003(gpu, case, family):
    """A last workgroup of the wave kernel with three of its four waves idle, and a tree grid of nq * groups workgroups."""
    assert case[3] == 1003 and case[3] % 4 == 3
    _check_case(gpu, *case, family)


def test_negative_count_in_the_first_list_is_an_empty_list(gpu):
    """The case the skip 'this query's row is already final' of the search's own merge launches used to leak into: plain
    layout, list 0 of a query has a negative count.  Hand-written, both final kernels and a tree."""
    for n_lists, k in ((3, 4), (2, 200), (9, 1000)):
        doc = np.arange(2 * n_lists * k, dtype=np.int32).reshape(2, n_lists, k) * 7 + 1
        score = (1.0 + (np.arange(2 * n_lists * k, dtype=np.float32) * 37 % 101)).reshape(2, n_lists, k)
        count = np.full((2, n_lists), k, np.int32)
        count[0, 0], count[1, 0] = -1, -2 ** 31
        lists = (doc, score, count)
        exp = packed_rows(merge(lists, k))
        assert exp[0, 2 * k] == min(k, (n_lists - 1) * k)
        for layout in LAYOUTS:
            _same(_run_layout(gpu, layout, lists, k, f"first count negative {n_lists}x{k}"), exp, f"{n_lists}x{k} [{layout}]")


@pytest.mark.parametrize("case,family", [((8, 128, "wave", 5), "unordered"), ((41, 100, "tree1+wave", 9), "ties"),
                                         ((17, 1024, "tree2+block", 4), "dirty")], ids=["wave", "tree1", "tree2"])
def test_merge_on_a_side_stream(gpu, case, family):
    """Inputs, outputs and the merge on a stream of the test's, behind a sleep; only that stream is synchronised."""
    torch, _, dev = gpu
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        torch.cuda._sleep(20_000_000)
        _check_case(gpu, *case, family, stream=s)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case,family", [((16, 64, "wave", 9), "dirty"), ((40, 100, "block", 5), "dirty"),
                                         ((41, 100, "tree1+wave", 9), "dirty"), ((65, 1024, "tree3+block", 3), "ties")],
                         ids=["wave", "block", "tree1", "tree3"])
def test_python_wrappers(gpu, case, family):
    """merge_topk_device (both layouts), merge_topk_packed_device and merge_topk_packed_out_device: outputs they allocate."""
    torch, _, dev = gpu
    from sparse_rx.index import merge_topk_device, merge_topk_packed_device, merge_topk_packed_out_device
    n_lists, k, want, nq = case
    assert bucket(n_lists, k) == want
    lists = make_input(family, nq, n_lists, k, case_seed(n_lists, k, nq, family))
    exp = packed_rows(merge(lists, k))
    as_f32 = lambda t: t.view(torch.float32)  # noqa: E731
    for gathered in (False, True):
        d, s, c = (_upload(torch, dev, a) for a in (to_gathered(lists) if gathered else to_plain(lists)))
        out = merge_topk_device(d, as_f32(s), c, k, gathered=gathered)
        torch.cuda.synchronize()
        got = np.concatenate([_words(out[0].cpu().numpy()), _words(out[1].cpu().numpy()), out[2].cpu().numpy()[:, None]], axis=1)
        _same(got, exp, f"merge_topk_device gathered={gathered}")
    p = _upload(torch, dev, to_packed(lists))
    out = merge_topk_packed_device(p, k)
    torch.cuda.synchronize()
    got = np.concatenate([_words(out[0].cpu().numpy()), _words(out[1].cpu().numpy()), out[2].cpu().numpy()[:, None]], axis=1)
    _same(got, exp, "merge_topk_packed_device")
    rows = merge_topk_packed_out_device(p, k)
    torch.cuda.synchronize()
    _same(rows.cpu().numpy(), exp, "merge_topk_packed_out_device")
