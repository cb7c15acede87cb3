"""Field collapsing on the GPU (include/sparse_rx_collapse.h).  Expected rows are never the engine's own: the restatement
(tests/collapse_ref.py) on the column and the lists a call was given.  Every comparison is exact -- doc ids, positions, group
sizes, counts and the BITS of the scores --, and every output buffer is pre-filled with 0x7f bytes so that a word the kernel
does not write shows."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import collapse_ref  # noqa: E402
from collapse_ref import NULL_DROP, NULL_ONE, NULL_OWN  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -(2 ** 31), 2 ** 31 - 1, -(2 ** 63), 2 ** 63 - 1
GARBAGE = 0x7F7F7F7F
N_DOCS, BASE = 6001, 1000  # an odd table with a doc_base: global ids are BASE .. BASE + N_DOCS - 1


class _Column:
    """One column on the device, as the C call takes it, next to its host arrays"""

    def __init__(self, keys, valid=None, n_docs=None, doc_base=0):
        import torch
        from sparse_rx import _capi
        from sparse_rx.filter import pack_masks
        self.keys = np.ascontiguousarray(keys)
        assert self.keys.dtype in (np.int32, np.int64)
        self.valid = None if valid is None else np.asarray(valid, dtype=bool)
        self.n_docs, self.doc_base = len(self.keys) if n_docs is None else n_docs, doc_base
        self.data_t = torch.from_numpy(self.keys).to(DEVICE)
        self.valid_t = None if valid is None else torch.from_numpy(pack_masks(self.valid).view(np.int32).copy()).to(DEVICE).reshape(-1)
        self.desc = _capi.FieldColDesc(data=self.data_t.data_ptr(), valid=None if valid is None else self.valid_t.data_ptr(),
                                       type=_capi.SRX_FIELD_I64 if self.keys.dtype == np.int64 else _capi.SRX_FIELD_I32)

    def run(self, doc, score, count, k, per_group=1, policy=NULL_OWN, pos=True, size=True, stream=None, outs=None):
        """The C call on fresh (or the given) garbage-filled outputs -> host (doc, score, count, pos | None, size | None), and the
        device outputs"""
        import ctypes
        import torch
        from sparse_rx import _capi
        nq, m = doc.shape
        d_t, s_t = torch.from_numpy(np.ascontiguousarray(doc, dtype=np.int32)).to(DEVICE), torch.from_numpy(np.ascontiguousarray(score, dtype=np.float32)).to(DEVICE)
        c_t = None if count is None else torch.from_numpy(np.ascontiguousarray(count, dtype=np.int32)).to(DEVICE)
        if outs is None:
            outs = [torch.full((nq, k), GARBAGE, dtype=torch.int32, device=DEVICE) for _ in range(4)] + [torch.full((nq,), GARBAGE, dtype=torch.int32, device=DEVICE)]
        o_doc, o_score, o_pos, o_size, o_count = outs
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        rc = _capi.lib().srx_collapse_topk(0, ctypes.byref(self.desc), self.n_docs, self.doc_base, ptr(d_t), ptr(s_t), ptr(c_t), nq, m, k, per_group, policy,
                                           ptr(o_doc), ptr(o_score), ptr(o_count), ptr(o_pos) if pos else None, ptr(o_size) if size else None, sp)
        _capi.check(rc, "srx_collapse_topk")
        torch.cuda.synchronize()
        host = [o_doc.cpu().numpy(), o_score.cpu().numpy().view(np.float32), o_count.cpu().numpy(), o_pos.cpu().numpy(), o_size.cpu().numpy()]
        return host, outs

    def expect(self, doc, score, count, k, per_group=1, policy=NULL_OWN):
        return collapse_ref.collapse(self.keys, self.valid, self.n_docs, self.doc_base, doc, score, count, k, per_group, policy)

    def check(self, doc, score, count, k, per_group=1, policy=NULL_OWN, pos=True, size=True, label="", **kw):
        got, outs = self.run(doc, score, count, k, per_group, policy, pos, size, **kw)
        exp = self.expect(doc, score, count, k, per_group, policy)
        names = ("doc", "score", "count", "pos", "group_size")
        for name, g, e, given in zip(names, got, exp, (True, True, True, pos, size)):
            if given:
                assert np.array_equal(g.view(np.int32), e.view(np.int32)), (label, name, k, per_group, policy)
            else:  # an output that was not given is not touched
                assert (g.view(np.int32) == GARBAGE).all(), (label, name)
        return got, exp, outs


def _lists(rng, nq, m, n_docs=N_DOCS, base=BASE, dead=0.05):
    """nq lists of m distinct docs of the table, a few positions replaced by ids outside it; scores are random BITS"""
    doc = np.empty((nq, m), dtype=np.int64)
    for q in range(nq):
        doc[q] = rng.choice(n_docs, size=m, replace=False) + base
    outside = np.array([-1, base - 1, base + n_docs, base + n_docs + 7, 0, I32_MAX, I32_MIN], dtype=np.int64)
    hit = rng.random((nq, m)) < dead
    doc[hit] = rng.choice(outside, size=int(hit.sum()))
    score = rng.integers(0, 2 ** 32, size=(nq, m), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return doc.astype(np.int32), score


@pytest.fixture(scope="module")
def col():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()
    rng = np.random.default_rng(1)
    keys = rng.integers(0, N_DOCS // 3, N_DOCS).astype(np.int64) - 500  # about 3 docs per key
    valid = rng.random(N_DOCS) > 0.1
    return _Column(keys, valid, doc_base=BASE)


# ---- 1. geometries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048])
def test_geometry(col, m):
    rng = np.random.default_rng(m)
    ks = sorted({1, min(2, m), max(m - 1, 1), m})
    groups = [1, 2, m, I32_MAX]
    for nq in (1, 3, 67):
        doc, score = _lists(rng, nq, m)
        count = rng.integers(0, m + 1, nq).astype(np.int32)
        count[0] = m
        combos = [(k, g) for k in ks for g in groups] if nq == 3 else [(k, groups[(i + nq) % 4]) for i, k in enumerate(ks)]
        for i, (k, g) in enumerate(combos):
            col.check(doc, score, count if i % 2 else None, k, g, (NULL_OWN, NULL_ONE, NULL_DROP)[i % 3], label=f"m={m} nq={nq}")


def test_many_queries(col):
    rng = np.random.default_rng(7)
    doc, score = _lists(rng, 70_000, 4)
    count = rng.integers(-1, 6, 70_000).astype(np.int32)
    got, exp, _ = col.check(doc, score, count, 3, 1, NULL_ONE, label="nq=70000")
    assert 0 < int((exp[2] == 3).sum()) < 70_000


# ---- 2. keys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_key_values(dtype):
    rng = np.random.default_rng(11)
    n, m = 3000, 300
    lo, hi = (I32_MIN, I32_MAX) if dtype == np.int32 else (I64_MIN, I64_MAX)
    pool = [lo, lo + 1, -1, 0, 1, hi - 1, hi]
    if dtype == np.int64:
        pool += [1 << 32, 2 << 32, (1 << 32) + 5, 5, -(1 << 32), (-(1 << 32)) + 5, 1 << 62, -(1 << 62)]  # equal low words, other high words
    keys = np.array([pool[i] for i in rng.integers(0, len(pool), n)], dtype=dtype)
    c = _Column(keys, None)
    doc, score = _lists(rng, 5, m, n_docs=n, base=0)
    for g in (1, 2, I32_MAX):
        got, exp, _ = c.check(doc, score, None, m, g, label=f"limits {dtype.__name__}")
    assert int(exp[2].max()) > len(pool)  # per_group = INT32_MAX keeps every live position
    _, exp, _ = c.check(doc, score, None, m, 1, label="limits")
    assert sorted(set(exp[2].tolist())) == [len(pool)]  # every key of the pool is a group of its own: none was folded into another
    # all keys equal, all distinct
    for keys, survivors in ((np.full(n, 7, dtype=dtype), 1), (np.arange(n).astype(dtype) - 1500, None)):
        c = _Column(keys, None)
        doc, score = _lists(rng, 3, m, n_docs=n, base=0, dead=0.0)
        _, exp, _ = c.check(doc, score, None, m, 1, label="equal / distinct")
        assert exp[2].tolist() == [m if survivors is None else survivors] * 3
        c.check(doc, score, None, m - 1, 2, label="equal / distinct")


@pytest.mark.parametrize("m", [2048, 1000, 300])
def test_group_on_block_borders(m):
    """One group whose members are the first and last position of the list and of every 64- (hence every 256-) position block;
    every other position is a group of its own"""
    n = 8192
    keys = np.arange(n, dtype=np.int64) + (1 << 40)
    doc = np.arange(m, dtype=np.int32)[None].repeat(2, 0) + 11
    doc[1] = doc[1][::-1] + 4000  # another list: other docs at the same places
    border = [p for p in range(m) if p % 64 in (0, 63) or p == m - 1]
    for q in range(2):
        keys[doc[q, border]] = -9
    c = _Column(keys, None)
    score = np.linspace(5, 1, 2 * m).astype(np.float32).reshape(2, m)
    for g, k in ((1, m), (2, m), (len(border) - 1, m), (I32_MAX, m), (3, 70), (1, 1)):
        got, exp, _ = c.check(doc, score, None, k, g, label=f"borders m={m}")
        assert exp[4][0, 0] == len(border) and exp[2][0] == min(k, m - len(border) + min(g, len(border)))


# ---- 3. validity rows, null policies ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [NULL_OWN, NULL_ONE, NULL_DROP])
def test_validity_rows(policy):
    rng = np.random.default_rng(13)
    n, m = 1000, 200
    keys = rng.integers(0, 40, n).astype(np.int32)
    cases = {"first and last without": np.ones(n, bool), "only first and last with": np.zeros(n, bool), "none with": np.zeros(n, bool),
             "random": rng.random(n) > 0.5}
    cases["first and last without"][[0, n - 1]] = False
    cases["only first and last with"][[0, n - 1]] = True
    doc, score = _lists(rng, 4, m, n_docs=n, base=50)
    doc[:, 3], doc[:, m - 2] = 50, 50 + n - 1  # the first and the last doc of the table are in every list
    for label, valid in cases.items():
        c = _Column(keys, valid, doc_base=50)
        for g in (1, 2):
            got, exp, _ = c.check(doc, score, None, m, g, policy, label=label)
        if label == "none with":
            live = int(((doc[0] >= 50) & (doc[0] < 50 + n)).sum())
            assert exp[2][0] == (live if policy == NULL_OWN else min(2, live) if policy == NULL_ONE else 0)


# ---- 4. counts, dead positions, scores, optional outputs -------------------------------------------------------------------------
def test_counts_and_dead_positions(col):
    rng = np.random.default_rng(17)
    m = 130
    doc, score = _lists(rng, 7, m, dead=0.0)
    count = np.array([-3, 0, m, m + 50, 1, 65, I32_MIN], dtype=np.int32)
    col.check(doc, score, count, m, 1, label="counts")
    col.check(doc, score, None, m, 1, label="no counts")
    # a dead position between two members of a group must not count as earlier: A dead A A with per_group = 2
    keys = np.zeros(10, dtype=np.int64)
    c = _Column(keys, None, doc_base=100)
    for dead_id in (-1, 99, 110, 5, I32_MAX, I32_MIN):
        d = np.array([[100, dead_id, 101, 102, 109, dead_id]], dtype=np.int32)
        got, exp, _ = c.check(d, np.arange(6, dtype=np.float32)[None], None, 6, 2, label=f"dead {dead_id}")
        assert got[3][0, :2].tolist() == [0, 2] and got[2].tolist() == [2] and got[4][0, :2].tolist() == [4, 4]
    # the table's first and last doc are live, their neighbours outside are not
    d = np.array([[99, 100, 109, 110]], dtype=np.int32)
    got, _, _ = c.check(d, np.zeros((1, 4), np.float32), None, 4, 4, label="edges")
    assert got[0][0].tolist() == [100, 109, -1, -1]


def test_scores_are_copied_as_bits(col):
    bits = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0xBF800000, 0x00000001, 0x7FA00000, 0xC2F70000], dtype=np.uint32)
    rng = np.random.default_rng(19)
    doc, _ = _lists(rng, 3, len(bits), dead=0.0)
    score = np.stack([bits, bits[::-1], np.roll(bits, 3)]).view(np.float32)
    got, exp, _ = col.check(doc, score, None, len(bits), I32_MAX, label="bits")
    assert np.array_equal(got[1].view(np.uint32), score.view(np.uint32))  # every position survives: the scores come back bit for bit


@pytest.mark.parametrize("pos,size", [(True, True), (False, False), (True, False), (False, True)])
def test_optional_outputs(col, pos, size):
    rng = np.random.default_rng(23)
    for m, k in ((50, 7), (700, 700)):
        doc, score = _lists(rng, 5, m)
        col.check(doc, score, None, k, 2, NULL_ONE, pos=pos, size=size, label="optional")


def test_side_stream_and_second_call(col):
    import torch
    rng = np.random.default_rng(29)
    doc, score = _lists(rng, 9, 600)
    side = torch.cuda.Stream(device=DEVICE)
    _, _, outs = col.check(doc, score, None, 40, 1, label="side stream", stream=side)
    # a second call into the same buffers, another list and another rule: nothing of the first call is left
    doc2, score2 = _lists(rng, 9, 600, dead=0.6)
    count2 = rng.integers(0, 100, 9).astype(np.int32)
    col.check(doc2, score2, count2, 40, 3, NULL_DROP, label="second call", outs=outs)
    col.check(doc, score, None, 40, 1, label="third call", stream=side, outs=outs)


# ---- 5. the Python doors ---------------------------------------------------------------------------------------------------------
def test_field_table_doors():
    import torch
    import sparse_rx
    rng = np.random.default_rng(31)
    n, m = 500, 90
    parent = rng.integers(0, 60, n).astype(np.int64) << 33
    year = np.ma.masked_array(rng.integers(2000, 2010, n).astype(np.int32), mask=rng.random(n) < 0.3)
    src = [None if rng.random() < 0.2 else ["wiki", "arxiv", "web", "news"][int(rng.integers(0, 4))] for _ in range(n)]
    table = sparse_rx.FieldTable.from_columns({"parent": parent, "year": year, "src": src, "price": np.ones(n, np.float32)}, device=DEVICE, doc_base=20)
    doc, score = _lists(rng, 6, m, n_docs=n, base=20)
    count = rng.integers(0, m + 1, 6).astype(np.int32)
    for name in ("parent", "year", "src"):
        hc = table.columns[name]
        for nulls in ("own", "one", "drop"):
            exp = collapse_ref.collapse(hc.data, hc.valid, n, 20, doc, score, count, 10, 2, collapse_ref.POLICY[nulls])
            got = table.collapse(name, doc, score, count, 10, per_group=2, nulls=nulls, want_pos=True, want_group_size=True)
            assert len(got) == 5
            for g, e in zip(got, exp):
                assert np.array_equal(g.view(np.int32), e.view(np.int32)), (name, nulls)
            dev = table.collapse_device(name, torch.from_numpy(doc).to(DEVICE), torch.from_numpy(score).to(DEVICE), None, 10, nulls=nulls, want_group_size=True)
            exp = collapse_ref.collapse(hc.data, hc.valid, n, 20, doc, score, None, 10, 1, collapse_ref.POLICY[nulls])
            assert len(dev) == 4 and all(t.device == table.device for t in dev)
            for g, e in zip(dev, (exp[0], exp[1], exp[2], exp[4])):
                assert np.array_equal(g.cpu().numpy().view(np.int32), e.view(np.int32)), (name, nulls)
    assert len(table.collapse("src", doc, score, None, 10)) == 3
    with pytest.raises(ValueError, match="'price' is a float column"):
        table.collapse("price", doc, score, None, 10)
    with pytest.raises(ValueError, match="is on cpu"):
        table.collapse_device("parent", torch.from_numpy(doc), torch.from_numpy(score), None, 10)
    table.close()


@pytest.fixture(scope="module")
def text(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    ids = list(j["corpus"])
    parent = [None if i % 11 == 5 else i // 4 for i in range(len(ids))]  # chunks of four, a few docs without a parent
    src = ["wiki", "arxiv", "web"]
    return j, ids, {"parent": parent, "src": [src[(i * 7) % 3] for i in range(len(ids))], "price": np.ones(len(ids), np.float32)}


def _expected_rows(ids_in_order, key_of, top_k, per_group=1, nulls="own"):
    """The restatement over one list of doc ids: key_of[doc id] is the key (an int, or a category's string), or None"""
    n = len(ids_in_order)
    number = {}  # a string's number: any numbering that keeps distinct strings apart
    keys = [0 if key_of[d] is None else key_of[d] if not isinstance(key_of[d], str) else number.setdefault(key_of[d], len(number)) for d in ids_in_order]
    valid = [key_of[d] is not None for d in ids_in_order]
    rows = collapse_ref.collapse_list(keys, valid, n, 0, list(range(n)), [0] * n, None, top_k, per_group, collapse_ref.POLICY[nulls])
    return [ids_in_order[r[2]] for r in rows]


def test_service_collapse_over_any_result(text):
    import sparse_rx
    j, ids, columns = text
    queries = dict(j["queries"])
    rng = np.random.default_rng(37)
    dim = 64
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    with pytest.raises(ValueError, match=r"collapse\(\.\.\.\) needs the docs' fields"):
        svc.collapse({"q0": {ids[0]: 1.0}}, "parent")
    svc.set_doc_fields(columns)
    svc.set_embeddings(rng.standard_normal((len(ids), dim)).astype(np.float32))
    svc.set_token_embeddings({d: rng.standard_normal((3, 32)).astype(np.float32) for d in ids})
    parent_of, src_of = dict(zip(ids, columns["parent"])), dict(zip(ids, columns["src"]))
    sparse = svc.search_bm25(queries, top_k=60)
    late = svc.rerank_late(sparse, {q: rng.standard_normal((4, 32)).astype(np.float32) for q in queries}, top_k=40)
    vec = {"v": svc.search_by_vector(rng.standard_normal(dim).astype(np.float32), k=50, min_score=-100.0)}
    for results in (sparse, late, {**sparse, "empty": {}}):
        for by, key_of, kw in (("parent", parent_of, dict(top_k=10)), ("parent", parent_of, dict(top_k=7, per_group=2, nulls="one")),
                               ("parent", parent_of, dict(top_k=100, nulls="drop")), ("src", src_of, dict(top_k=5, per_group=2))):
            got = svc.collapse(results, by, **kw)
            assert list(got) == list(results)
            for q, row in results.items():
                want = _expected_rows(list(row), key_of, kw["top_k"], kw.get("per_group", 1), kw.get("nulls", "own"))
                assert list(got[q].items()) == [(d, row[d]) for d in want], (by, kw, q)
    assert any(len(v) == 10 for v in svc.collapse(sparse, "parent").values())
    assert any(list(svc.collapse(sparse, "parent")[q]) != list(sparse[q])[:10] for q in sparse)  # something was collapsed
    got = svc.collapse(vec, "parent", top_k=12)
    by_id = {r["doc_id"]: r for r in vec["v"]}
    assert got["v"] == [by_id[d] for d in _expected_rows([r["doc_id"] for r in vec["v"]], parent_of, 12)] and len(got["v"]) == 12
    assert svc.collapse({}, "parent") == {} and svc.collapse(sparse, "parent", top_k=0) == {q: {} for q in sparse}
    with pytest.raises(ValueError, match="unknown doc id"):
        svc.collapse({"q0": {"no such doc": 1.0}}, "parent")
    with pytest.raises(ValueError, match="at most 2048 docs"):  # the corpus is smaller than that: the list form can name a doc twice
        svc.collapse({"v": [{"doc_id": ids[i % len(ids)], "score": 1.0} for i in range(2049)]}, "parent")
    svc.close()


# ---- 6. the exact paged door ----------------------------------------------------------------------------------------------------
def test_search_bm25_collapse_is_exact_over_the_complete_ranking(tmp_path):
    import sparse_rx
    n, n_all = 3000, 6500
    rng = np.random.default_rng(41)
    # 3 000 docs hold the query's word (fewer than half of the corpus: its idf is positive); lengths and a second word vary, so the
    # ranking has many distinct scores and long runs of ties
    corpus = {f"d{i}": {"text": " ".join(["common"] * (1 + i % 3) * (i < n) + ["rare"] * (i % 5 == 0 and i < n) + ["pad"] * int(rng.integers(1, 40)))}
              for i in range(n_all)}
    queries = {"qa": "common rare", "qb": "common", "blank": "  "}
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=8)
    svc.build_bm25_index(corpus)
    full = svc.search_bm25(queries, top_k=n_all)
    assert len(full["qa"]) == n == len(full["qb"]) and full["blank"] == {}
    ranking = list(full["qa"])
    row = {d: i for i, d in enumerate(corpus)}
    parent = np.arange(10_000, 10_000 + n_all, dtype=np.int64)
    parent[[row[d] for d in ranking[:2500]]] = 42  # ranks 1 .. 2500 of qa are one group
    flag = (np.arange(n_all) % 3 != 0).astype(np.int32)
    svc.set_doc_fields({"parent": parent, "flag": flag})
    key_of = {d: int(parent[row[d]]) for d in corpus}
    cached = len(svc.query_cache)

    def want(q, docs, k, g):
        return [(d, full[q][d]) for d in _expected_rows(docs, key_of, k, g)]

    for g in (1, 3):
        got = svc.search_bm25(queries, top_k=5, collapse_by="parent", per_group=g)
        for q in ("qa", "qb"):
            assert list(got[q].items()) == want(q, list(full[q]), 5, g), (q, g)
        assert len(got["qa"]) == 5 and got["blank"] == {}
        assert list(got["qa"])[:g] == ranking[:g] and set(list(got["qa"])[g:]) <= set(ranking[2500:])
    # under excluded_docs= and where=: the collapsed ranking of the allowed docs
    out = ranking[:3] + ranking[2500:2502] + ranking[100:120]
    got = svc.search_bm25(queries, top_k=5, collapse_by="parent", excluded_docs=out)
    for q in ("qa", "qb"):
        assert list(got[q].items()) == want(q, [d for d in full[q] if d not in set(out)], 5, 1), q
    got = svc.search_bm25(queries, top_k=5, collapse_by="parent", per_group=2, where={"must": [{"field": "flag", "eq": 1}]})
    for q in ("qa", "qb"):
        assert list(got[q].items()) == want(q, [d for d in full[q] if flag[row[d]] == 1], 5, 2), q
    # a depth limit returns what the rows read so far hold
    got = svc.search_bm25(queries, top_k=5, collapse_by="parent", collapse_depth=1500)
    assert list(got["qa"].items()) == want("qa", ranking[:1500], 5, 1) and len(got["qa"]) == 1
    assert len(svc.query_cache) == cached  # none of these calls read or wrote the cache
    assert svc.search_bm25(queries, top_k=5) == {q: dict(list(full[q].items())[:5]) for q in queries}
    with pytest.raises(ValueError, match="at most 1024 rows"):
        svc.search_bm25(queries, top_k=1025, collapse_by="parent")
    # the registry mirrors go through the same backend function
    r = sparse_rx.OptimizedBM25Retriever(device=DEVICE, tile_log2=8)
    r.build_index_from_corpus(corpus)
    r.set_doc_fields({"parent": parent})
    got = r.search({"qa": queries["qa"]}, top_k=5, collapse_by="parent", per_group=3)
    assert list(got["qa"].items()) == want("qa", ranking, 5, 3) and len(r.query_cache) == 0
    r.close()
    p = sparse_rx.OptimizedRetriever({"type": "bm25"}, device=DEVICE, tile_log2=8, cache_dir=str(tmp_path))
    p.build_index_from_corpus(corpus)
    p.set_doc_fields({"parent": parent})
    pfull = p.search({"qb": queries["qb"]}, top_k=n_all)["qb"]  # its own accumulation order, its own floats
    got = p.search({"qb": queries["qb"]}, top_k=5, collapse_by="parent")
    assert list(got["qb"].items()) == [(d, pfull[d]) for d in _expected_rows(list(pfull), key_of, 5, 1)]
    p.close()
    svc.close()


# ---- 7. the hybrid mirror on tests/golden/text_small.json --------------------------------------------------------------------------
def test_search_hybrid_collapse_equals_its_chain(text):
    import sparse_rx
    j, ids, columns = text
    queries = {q: j["queries"][q] for q in list(j["queries"])[:12]}
    n_docs, dim = len(ids), 96
    rng = np.random.default_rng(43)
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    svc.set_embeddings(rng.standard_normal((n_docs, dim)).astype(np.float32))
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    with pytest.raises(ValueError, match=r"search_hybrid\(collapse_by=\.\.\.\) needs the docs' fields"):
        svc.search_hybrid(queries, vecs, top_k=5, collapse_by="parent")
    svc.set_doc_fields(columns)
    same = lambda a, b: {q: list(v.items()) for q, v in a.items()} == {q: list(v.items()) for q, v in b.items()}
    for extra in (dict(), dict(rescore=True), dict(fusion="rrf"), dict(excluded_docs=ids[:40])):
        for kw in (dict(collapse_by="parent"), dict(collapse_by="src", per_group=2), dict(collapse_by="parent", collapse_nulls="drop", per_group=3)):
            args = dict(by=kw["collapse_by"], per_group=kw.get("per_group", 1), nulls=kw.get("collapse_nulls", "own"))
            got = svc.search_hybrid(queries, vecs, top_k=5, collapse_pool=40, **kw, **extra)
            pool = svc.search_hybrid(queries, vecs, top_k=40, **extra)
            assert same(got, svc.collapse(pool, top_k=5, **args)), (extra, kw)
            if kw["collapse_by"] == "src":  # three sources, two docs of each: a top five with three docs of one source does not survive
                assert any(list(got[q]) != list(pool[q])[:5] for q in queries), (extra, kw)
        got = svc.search_hybrid(queries, vecs, top_k=5, collapse_by="parent", **extra)  # the default pool: min(max(20, 100), 1024, n_docs)
        assert same(got, svc.collapse(svc.search_hybrid(queries, vecs, top_k=100, **extra), "parent", top_k=5)), extra
    # a pool that holds fewer groups than top_k: a shorter list, not an error
    got = svc.search_hybrid(queries, vecs, top_k=5, collapse_by="src", collapse_pool=8)
    assert all(len(v) <= 3 for v in got.values()) and same(got, svc.collapse(svc.search_hybrid(queries, vecs, top_k=8), "src", top_k=5))
    with pytest.raises(ValueError, match="collapse_pool must be in"):
        svc.search_hybrid(queries, vecs, top_k=5, collapse_by="parent", collapse_pool=1025)
    with pytest.raises(ValueError, match="'price' is a float column"):
        svc.search_hybrid(queries, vecs, top_k=5, collapse_by="price")
    # MMR: fuse collapse_pool deep, collapse to mmr_pool, pick top_k
    for extra in (dict(), dict(rescore=True)):
        got = svc.search_hybrid(queries, vecs, top_k=5, collapse_by="parent", collapse_pool=40, mmr_lambda=0.5, mmr_pool=12, **extra)
        chain = svc.diversify(svc.collapse(svc.search_hybrid(queries, vecs, top_k=40, **extra), "parent", top_k=12), top_k=5, mmr_lambda=0.5)
        assert same(got, chain) and all(len(v) == 5 for v in got.values()), extra
    # late interaction: fuse late_pool deep, rerank the whole pool, collapse to top_k
    svc.set_token_embeddings({d: rng.standard_normal((3, 32)).astype(np.float32) for d in ids})
    qt = {q: rng.standard_normal((4, 32)).astype(np.float32) for q in queries}
    for extra in (dict(), dict(rescore=True)):
        got = svc.search_hybrid(queries, vecs, top_k=5, collapse_by="parent", per_group=2, late_query_tokens=qt, late_pool=30, **extra)
        chain = svc.collapse(svc.rerank_late(svc.search_hybrid(queries, vecs, top_k=30, **extra), qt, top_k=30), "parent", top_k=5, per_group=2)
        assert same(got, chain) and all(len(v) == 5 for v in got.values()), extra
    # without the keyword nothing changes
    assert same(svc.search_hybrid(queries, vecs, top_k=5, collapse_by=None, per_group=7), svc.search_hybrid(queries, vecs, top_k=5))
    svc.close()
