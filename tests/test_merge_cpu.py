"""The top-k merge without a GPU: the NumPy restatement (tests/merge_ref.py) on hand-written rows, its dispatch pinned to
the library through srx_merge_workspace_bytes (host-only) for every k, the argument checks of the four merge entry points
(none reaches a device) and the bucket of every row of the shape table tests/test_merge_gpu.py runs."""
import numpy as np
import pytest

import merge_ref
from merge_ref import BIG_CASES, BIG_FAMILIES, CASES, DOC_MAX, bucket, case_families, case_seed, dispatch, make_input, merge

INF, NAN, DEN, FMAX = np.float32(np.inf), np.float32(np.nan), np.float32(1e-45), np.float32(3.4028235e38)


def _lists(rows, k):
    """One query from [(docs, scores, count), ...]; short rows are filled with clean padding."""
    doc = np.full((1, len(rows), k), -1, np.int32)
    score = np.zeros((1, len(rows), k), np.float32)
    count = np.zeros((1, len(rows)), np.int32)
    for l, (d, s, c) in enumerate(rows):
        doc[0, l, :len(d)], score[0, l, :len(s)], count[0, l] = d, s, c
    return doc, score, count


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatement itself
# ---------------------------------------------------------------------------------------------------------------
def test_merge_hand_written_rows():
    # two ordered lists, a tie at 2.0 across them (doc 3 before doc 9), cut at k
    d, s, c = merge(_lists([([9, 4], [2.0, 1.0], 2), ([7, 3, 5], [3.0, 2.0, 0.5], 3)], 3), 3)
    assert d.tolist() == [[7, 3, 9]] and s.tolist() == [[3.0, 2.0, 2.0]] and c.tolist() == [3]
    # fewer than k entries: padded with -1 / +0.0, count = what there is
    d, s, c = merge(_lists([([9], [2.0], 1), ([], [], 0), ([1], [5.0], 1)], 4), 4)
    assert d.tolist() == [[1, 9, -1, -1]] and c.tolist() == [2]
    assert _bits(s).tolist() == [_bits([5.0, 2.0, 0.0, 0.0]).tolist()]
    # the tie group at the boundary spans three lists: the smallest doc ids win, whatever list or slot they sit in
    d, s, c = merge(_lists([([50, 10], [1.0, 1.0], 2), ([40, 60], [1.0, 7.0], 2), ([20, 30], [1.0, 1.0], 2)], 3), 3)
    assert d.tolist() == [[60, 10, 20]] and s.tolist() == [[7.0, 1.0, 1.0]] and c.tolist() == [3]
    # nothing usable at all
    d, s, c = merge(_lists([([1, 2], [0.0, -1.0], 2), ([3], [9.0], 0)], 2), 2)
    assert d.tolist() == [[-1, -1]] and _bits(s).tolist() == [[0, 0]] and c.tolist() == [0]


def test_merge_counts_junk_and_special_scores():
    k = 4
    rows = [
        ([11, 12, 13, 14], [9.0, 8.0, 99.0, 98.0], 2),      # junk after count is not read
        ([21, 22, 23, 24], [1.0, 2.0, 3.0, 4.0], 7),        # count above k: k entries, order inside a list is irrelevant
        ([31, 32, 33, 34], [50.0, 51.0, 52.0, 53.0], -1),   # a negative count is an empty list
        ([41, 42, 43, 44], [0.0, -0.0, -5.0, NAN], 4),      # none of these is > 0
        ([0, DOC_MAX, 53, 54], [INF, DEN, FMAX, -INF], 4),  # +inf and denormals are kept; both ends of the id range
    ]
    d, s, c = merge(_lists(rows, k), k)
    assert d.tolist() == [[0, 53, 11, 12]] and c.tolist() == [4]
    assert _bits(s).tolist() == [_bits([INF, FMAX, 9.0, 8.0]).tolist()]
    # the lists hold 9 usable entries; the denormal is the last of them
    doc, score, count = _lists(rows, k)
    used = [(float(score[0, l, r]), int(doc[0, l, r])) for l in range(5) for r in range(min(max(int(count[0, l]), 0), k))
            if score[0, l, r] > 0]
    assert len(used) == 9 and min(used) == (float(DEN), DOC_MAX)
    # first list negative, as the only list and as one of two
    d, s, c = merge(_lists([([5], [3.0], -1)], 1), 1)
    assert d.tolist() == [[-1]] and c.tolist() == [0]
    d, s, c = merge(_lists([([5], [3.0], -2 ** 31), ([6], [2.0], 2 ** 31 - 1)], 1), 1)
    assert d.tolist() == [[6]] and s.tolist() == [[2.0]] and c.tolist() == [1]


@pytest.mark.parametrize("family,n_lists,k,nq", [(f, *c) for c in [(1, 7, 3), (8, 16, 5), (41, 100, 4), (5, 1024, 2)]
                                                 for f in case_families(c[0], ("distinct", "ties", "all_equal"))])
def test_merge_equals_a_lexsort_union_on_well_formed_inputs(family, n_lists, k, nq):
    doc, score, count = make_input(family, nq, n_lists, k, seed=17 * n_lists + k)
    assert count.min() >= 0 and count.max() <= k
    got = merge((doc, score, count), k)
    for q in range(nq):
        d = np.concatenate([doc[q, l, :count[q, l]] for l in range(n_lists)])
        s = np.concatenate([score[q, l, :count[q, l]] for l in range(n_lists)])
        assert (s > 0).all() and len(set(d.tolist())) == d.size
        order = np.lexsort((d, -s.astype(np.float64)))[:k]
        m = order.size
        assert got[2][q] == m
        assert np.array_equal(got[0][q, :m], d[order]) and np.array_equal(got[1][q, :m], s[order])
        assert (got[0][q, m:] == -1).all() and not got[1][q, m:].view(np.uint32).any()
        if family == "all_equal":
            assert np.array_equal(got[0][q], np.sort(doc[q].reshape(-1))[:k])


def test_layouts_hold_the_same_input():
    lists = make_input("dirty", 3, 5, 4, seed=1)
    doc, score, count = lists
    gd, gs, gc = merge_ref.to_gathered(lists)
    p = merge_ref.to_packed(lists)
    assert p.shape == (5, 3, 9) and p.dtype == np.int32 and p.flags.c_contiguous
    for q in range(3):
        for l in range(5):
            assert np.array_equal(gd[l, q], doc[q, l]) and gc[l, q] == count[q, l]
            assert np.array_equal(gs[l, q].view(np.uint32), score[q, l].view(np.uint32))
            assert np.array_equal(p[l, q, :4], doc[q, l]) and p[l, q, 8] == count[q, l]
            assert np.array_equal(p[l, q, 4:8].view(np.uint32), score[q, l].view(np.uint32))
    out = merge(lists, 4)
    rows = merge_ref.packed_rows(out)
    assert rows.shape == (3, 9) and np.array_equal(rows[:, :4], out[0]) and np.array_equal(rows[:, 8], out[2])
    assert np.array_equal(rows[:, 4:8].view(np.uint32), out[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# 2. the input families are what the GPU tests take them for
# ---------------------------------------------------------------------------------------------------------------
def _all_cases():
    return [(c, f) for c in CASES for f in case_families(c[0])] + [(c, f) for c in BIG_CASES for f in case_families(c[0], BIG_FAMILIES)]


def test_every_family_reaches_a_wave_case_a_block_case_and_every_tree_case():
    assert {c[3] for c in CASES} == {1, 3, 4, 5, 9}
    for f in merge_ref.FAMILIES:
        ran = {c[2] for c, g in _all_cases() if g == f}
        assert ran >= {c[2] for c in CASES}, f
    assert all("ties" in case_families(c[0]) for c in CASES if c[2].startswith("tree"))


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}" for c in CASES])
def test_input_families(case):
    n_lists, k, _, nq = case
    for family in case_families(n_lists):
        doc, score, count = lists = make_input(family, nq, n_lists, k, case_seed(n_lists, k, nq, family))
        assert doc.dtype == np.int32 and score.dtype == np.float32 and count.dtype == np.int32
        ref = merge(lists, k)
        for q in range(nq):  # no doc id twice in a query; ids within 0 .. 2^31 - 2, both ends present
            ids = doc[q].reshape(-1)
            ids = ids[ids != -1]
            assert np.unique(ids).size == ids.size and (ids.size == 0 or (ids.min() >= 0 and ids.max() <= DOC_MAX))
            if family in ("ties", "all_equal", "dirty") and n_lists * k >= 2:
                assert ids.min() == 0 and ids.max() == DOC_MAX
        if family == "ties":
            assert merge_ref.tie_boundary_ok(lists, k, dispatch(n_lists, k).fan).all()
        if family == "all_equal":
            assert np.array_equal(ref[0], np.sort(doc.reshape(nq, -1), axis=1)[:, :k])
        if family in ("distinct", "unordered") and nq > 1:
            assert (ref[2][1::2] < k).all() and (ref[0][1::2, -1] == -1).all()  # padding is checked
        if family == "distinct" and n_lists >= 2:
            assert (count[0] == 0).any() and (count[0] == k).any()
        if family == "dirty":
            assert (count[0::2, 0] < 0).all() and (np.isnan(score).any() or k * n_lists < 8)
            if n_lists >= 16:
                assert (count > k).any() and (count < 0).any()
        if family == "unordered" and k >= 16 and n_lists >= 2:
            s = score[0, int(np.argmax(count[0]))][: count[0].max()]
            assert (np.diff(s) > 0).any()  # not in rank order


# ---------------------------------------------------------------------------------------------------------------
# 3. the dispatch
# ---------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_pins_the_restated_tree_for_every_k():
    from sparse_rx import _capi
    L = _capi.lib()
    for k in range(1, 1025):
        fan = 4096 // k
        for n_lists in sorted({1, max(fan - 1, 1), fan, fan + 1, fan * fan, fan * fan + 1, 256, 257, 5000}):
            d = dispatch(n_lists, k)
            assert d.fan == fan and (n_lists <= fan) == (not d.levels)
            assert d.final_lists == (d.levels[-1] if d.levels else n_lists) and d.final_lists <= fan
            for nq in (1, 7, 10000):
                assert dispatch(n_lists, k, nq).workspace_bytes == L.srx_merge_workspace_bytes(nq, n_lists, k), (nq, n_lists, k)
    # the depth of the tree at the edges of the fan
    assert dispatch(16, 256).levels == () and dispatch(17, 256).levels == (2,)
    assert dispatch(256, 256).levels == (16,) and dispatch(257, 256).levels == (17, 2)
    assert dispatch(4096, 256).levels == (256, 16) and dispatch(4097, 256).levels == (257, 17, 2)


@pytest.mark.parametrize("case", CASES + BIG_CASES, ids=[f"{c[0]}x{c[1]}-nq{c[3]}" for c in CASES + BIG_CASES])
def test_shape_table_buckets(case):
    n_lists, k, want, nq = case
    assert bucket(n_lists, k) == want
    d = dispatch(n_lists, k, nq)
    assert (d.workspace_bytes > 0) == want.startswith("tree")
    if d.final == "wave":
        assert k <= 128 and d.final_lists * k <= 1024 and d.final_lists <= 256


def test_shape_table_is_the_issue_table():
    rows = {}
    for n_lists, k, b, _ in CASES:
        rows.setdefault(b, []).append((n_lists, k))
    assert rows == {
        "wave": [(1, 1), (1, 128), (8, 128), (16, 64), (10, 100), (256, 4), (256, 1)],
        "block": [(1, 129), (9, 128), (17, 64), (11, 100), (257, 3), (1024, 1), (4096, 1), (1, 1024), (4, 1024), (40, 100),
                  (31, 129), (3, 513), (4, 1000)],
        "tree1+wave": [(4097, 1), (41, 100)],
        "tree1+block": [(5, 1024), (16, 1024), (32, 129), (5, 1000)],
        "tree2+wave": [(1601, 100)],
        "tree2+block": [(17, 1024)],
        "tree3+block": [(65, 1024)],
    }


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals: nothing here reaches a device (the pointers are fakes: a launch would fault)
# ---------------------------------------------------------------------------------------------------------------
_A = dict(in_doc=1 << 20, in_score=1 << 21, in_count=1 << 22, packed=1 << 23, out_doc=1 << 24, out_score=1 << 25,
          out_count=1 << 26, out_packed=1 << 27, ws=1 << 28, ws_bytes=1 << 40, nq=4, n_lists=3, k=10)


def _call(entry, **kw):
    from sparse_rx import _capi
    L = _capi.lib()
    a = dict(_A)
    a.update(kw)
    if entry == "workspace_bytes":
        rc = L.srx_merge_workspace_bytes(a["nq"], a["n_lists"], a["k"])
    elif entry in ("plain", "gathered"):
        rc = L.srx_merge_topk(0, a["in_doc"], a["in_score"], a["in_count"], a["nq"], a["n_lists"], a["k"], int(entry == "gathered"),
                              a["out_doc"], a["out_score"], a["out_count"], a["ws"], a["ws_bytes"], None)
    elif entry == "packed":
        rc = L.srx_merge_topk_packed(0, a["packed"], a["nq"], a["n_lists"], a["k"], a["out_doc"], a["out_score"], a["out_count"],
                                     a["ws"], a["ws_bytes"], None)
    else:
        rc = L.srx_merge_topk_packed_out(0, a["packed"], a["nq"], a["n_lists"], a["k"], a["out_packed"], a["ws"], a["ws_bytes"], None)
    return rc, (L.srx_last_error() or b"")


_POINTERS = {"plain": ("in_doc", "in_score", "in_count", "out_doc", "out_score", "out_count"),
             "gathered": ("in_doc", "in_score", "in_count", "out_doc", "out_score", "out_count"),
             "packed": ("packed", "out_doc", "out_score", "out_count"), "packed_out": ("packed", "out_packed")}
_ENTRIES = ("plain", "gathered", "packed", "packed_out")


@pytest.mark.parametrize("entry", _ENTRIES + ("workspace_bytes",))
@pytest.mark.parametrize("bad", [dict(nq=-1), dict(n_lists=0), dict(n_lists=-1), dict(k=0), dict(k=-1), dict(k=1025)],
                         ids=lambda b: "{}={}".format(*next(iter(b.items()))))
def test_merge_refuses_bad_sizes(entry, bad):
    rc, msg = _call(entry, **bad)
    assert rc == -1 and msg.startswith(b"srx_merge_"), (entry, bad, rc, msg)
    if "nq" not in bad:  # nq == 0 does not excuse a bad size
        rc, msg = _call(entry, nq=0, **bad)
        assert rc == -1, (entry, bad, rc, msg)


@pytest.mark.parametrize("entry", _ENTRIES)
def test_merge_refuses_null_pointers(entry):
    for name in _POINTERS[entry]:
        rc, msg = _call(entry, **{name: None})
        assert rc == -1 and msg.startswith(b"srx_merge_topk"), (entry, name, rc, msg)


@pytest.mark.parametrize("entry", _ENTRIES)
@pytest.mark.parametrize("n_lists,k", [(41, 100), (5, 1024), (4097, 1), (65, 1024)])
def test_merge_workspace_null_or_short_is_nomem(entry, n_lists, k):
    need = dispatch(n_lists, k, _A["nq"]).workspace_bytes
    assert need > 0
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=None, ws_bytes=0)):
        rc, msg = _call(entry, n_lists=n_lists, k=k, **kw)
        assert rc == -3 and b"workspace too small" in msg, (entry, kw, rc, msg)


@pytest.mark.parametrize("entry", _ENTRIES + ("workspace_bytes",))
def test_merge_nq_zero_is_ok_without_a_launch(entry):
    assert _call(entry, nq=0)[0] == 0
    if entry == "workspace_bytes":
        assert _call(entry, nq=0, n_lists=5000, k=1024)[0] == dispatch(5000, 1024, 0).workspace_bytes == 512
        return
    assert _call(entry, nq=0, n_lists=5000, k=1024, ws=None, ws_bytes=0)[0] == 0  # no workspace asked of an empty batch
    # ... and no pointer looked at, but for the packed buffers, which the packed entry points check before the sizes
    assert _call(entry, nq=0, **{n: None for n in _POINTERS[entry] if "packed" not in n})[0] == 0
