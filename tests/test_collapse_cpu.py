"""Field collapsing without a GPU: the tenth header and its symbol table, every refusal of the entry point (none reaches a
device), the restatement (tests/collapse_ref.py) on a list worked by hand, the identity the paged door rests on, collapse_deep
over a fake search on CPU tensors, the Python refusals and the mirrors with no keyword given."""
import ctypes
import inspect
import json
import os
import re
import tempfile

import numpy as np
import pytest
import torch

import collapse_ref
import sparse_rx
from sparse_rx import _capi, fields
from sparse_rx.backend import CollapseSpec, collapse_deep, collapse_pool_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(16)]  # 16-byte aligned addresses, never dereferenced
I32_MAX = 2 ** 31 - 1


def test_tenth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_collapse.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.COLLAPSE_SYMBOLS) and len(declared) == 1, declared ^ set(_capi.COLLAPSE_SYMBOLS)
    assert '#include "sparse_rx_fields.h"' in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS, _capi.MMR_SYMBOLS,
              _capi.TERMS_SYMBOLS, _capi.MAXSIM_SYMBOLS, _capi.FIELDS_SYMBOLS)
    assert [len(t) for t in others] == [35, 4, 4, 8, 5, 3, 2, 3, 1]
    for other in others:
        assert not set(_capi.COLLAPSE_SYMBOLS) & set(other)
    assert sum(len(t) for t in others) + len(_capi.COLLAPSE_SYMBOLS) == 66
    assert "collapse.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "sparse_rx_collapse.h") in _capi._deps()
    assert "include/sparse_rx_collapse.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read().split('"""')[1]
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.COLLAPSE_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    for name, value in (("SRX_COLLAPSE_NULL_OWN", 0), ("SRX_COLLAPSE_NULL_ONE", 1), ("SRX_COLLAPSE_NULL_DROP", 2)):
        assert re.search(rf"\b{name} = {value}\b", hdr) and getattr(_capi, name) == value
        assert getattr(collapse_ref, name.split("_", 2)[2]) == value
    assert re.search(r"#define SRX_COLLAPSE_MAX_M 2048\b", hdr) and _capi.SRX_COLLAPSE_MAX_M == 2048 == collapse_ref.MAX_M
    assert fields.NULL_POLICIES == collapse_ref.POLICY
    assert sparse_rx.collapse_deep is collapse_deep and "collapse_deep" in sparse_rx.__all__


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, msg)


def _col(data, valid, typ):
    return ctypes.pointer(_capi.FieldColDesc(data=data, valid=valid, type=typ))


def test_entry_point_refusals():
    L = _capi.lib()
    ok = dict(device=0, col=_col(P[0], P[1], 1), n_docs=1000, doc_base=0, cand_doc=P[2], cand_score=P[3], cand_count=P[4], nq=3, m=100, k=10,
              per_group=1, null_policy=0, out_doc=P[5], out_score=P[6], out_count=P[7], out_pos=P[8], out_group=P[9], stream=None)
    call = lambda **kw: L.srx_collapse_topk(*{**ok, **kw}.values())
    _refused(call(col=None), "null col")
    for typ in (0, 1):
        _refused(call(col=_col(None, None, typ)), "null data")
    for typ, off in ((0, 2), (0, 1), (1, 4), (1, 2)):
        _refused(call(col=_col(P[0] + off, None, typ)), "aligned for its type")
    for typ in (2, 3, -1, 4):
        _refused(call(col=_col(P[0], None, typ)), "SRX_FIELD_I32 or SRX_FIELD_I64")
    for off in (4, 8, 2):
        _refused(call(col=_col(P[0], P[1] + off, 1)), "validity row must be 16-byte aligned")
    for n in (0, -3, 2 ** 31 - 1, 2 ** 40):
        _refused(call(n_docs=n), "n_docs must be in [1, 2^31 - 2]")
    _refused(call(doc_base=-1), "negative doc_base")
    for m in (0, -1, 2049, I32_MAX):
        _refused(call(m=m, k=1), "m must be in [1, 2048]")
    for k in (0, -1, 101, I32_MAX):
        _refused(call(k=k), "k must be in [1, m]")
    for g in (0, -1, -I32_MAX):
        _refused(call(per_group=g), "per_group must be >= 1")
    for pol in (-1, 3, 99):
        _refused(call(null_policy=pol), "unknown null_policy")
    _refused(call(nq=-1), "nq < 0")
    _refused(call(nq=(I32_MAX // 2048) + 1, m=2048), "nq * m")
    for name in ("cand_doc", "cand_score", "out_doc", "out_score", "out_count"):
        _refused(call(**{name: None}), "null ")
    assert b"srx_collapse_topk" in L.srx_last_error()
    # nothing to do: no launch, whatever the pointers are; the checks still come first
    assert call(nq=0) == 0
    assert call(nq=0, cand_doc=None, cand_score=None, cand_count=None, out_doc=None, out_score=None, out_count=None, out_pos=None, out_group=None) == 0
    assert call(nq=0, col=_col(P[0] + 4, None, 0), per_group=I32_MAX, m=2048, k=2048) == 0  # natural alignment is enough
    _refused(call(nq=0, k=0), "k must be in [1, m]")
    _refused(call(nq=0, col=_col(P[0], None, 2)), "SRX_FIELD_I32 or SRX_FIELD_I64")


# ---- the restatement on a list worked by hand -----------------------------------------------------------------------------------
def _hand():
    """20 docs, doc_base 100.  Key A = 7 at the local docs 3, 4, 6, 12; B = 9 at 5, 8, 13; C = -2 at 7, 9; the docs 10 and 11 have no
    value (their stored 7 must not show); the others a key of their own.  The list: positions 0..11 =
    A B null A dead A C null B C A B (position 4 names doc 300, outside the table)."""
    keys = np.array([100 + d for d in range(20)], dtype=np.int64)
    keys[[3, 4, 6, 12]], keys[[5, 8, 13]], keys[[7, 9]], keys[[10, 11]] = 7, 9, -2, 7
    valid = np.ones(20, bool)
    valid[[10, 11]] = False
    doc = np.array([[103, 105, 110, 104, 300, 106, 107, 111, 108, 109, 112, 113]], dtype=np.int32)
    score = np.array([[12 - i for i in range(12)]], dtype=np.float32)
    return keys, valid, doc, score


@pytest.mark.parametrize("per_group,policy,k,pos,sizes", [
    (1, "own", 12, [0, 1, 2, 6, 7], [4, 3, 1, 2, 1]),
    (1, "one", 12, [0, 1, 2, 6], [4, 3, 2, 2]),
    (1, "drop", 12, [0, 1, 6], [4, 3, 2]),
    (2, "own", 12, [0, 1, 2, 3, 6, 7, 8, 9], [4, 3, 1, 4, 2, 1, 3, 2]),
    (2, "one", 12, [0, 1, 2, 3, 6, 7, 8, 9], [4, 3, 2, 4, 2, 2, 3, 2]),
    (2, "drop", 12, [0, 1, 3, 6, 8, 9], [4, 3, 4, 2, 3, 2]),
    (2, "own", 4, [0, 1, 2, 3], [4, 3, 1, 4]),       # k cuts inside group A: its second member is the last row ...
    (2, "drop", 2, [0, 1], [4, 3]),                   # ... or is cut off, and the sizes do not change
    (3, "drop", 5, [0, 1, 3, 5, 6], [4, 3, 4, 4, 2]),
])
def test_restatement_by_hand(per_group, policy, k, pos, sizes):
    keys, valid, doc, score = _hand()
    d, s, c, p, g = collapse_ref.collapse(keys, valid, 20, 100, doc, score, None, k, per_group, collapse_ref.POLICY[policy])
    n = len(pos)
    assert c.tolist() == [n] and p[0, :n].tolist() == pos and g[0, :n].tolist() == sizes
    assert d[0, :n].tolist() == doc[0, pos].tolist() and s[0, :n].tolist() == score[0, pos].tolist()
    assert d[0, n:].tolist() == [-1] * (k - n) and p[0, n:].tolist() == [-1] * (k - n) and g[0, n:].tolist() == [0] * (k - n)
    assert s.view(np.uint32)[0, n:].tolist() == [0] * (k - n)


def test_restatement_counts_and_dead_positions():
    keys, valid, doc, score = _hand()
    own = collapse_ref.NULL_OWN
    # the count cuts the list: a negative one and 0 leave nothing, one above m means m
    for count, pos in ((-5, []), (0, []), (1, [0]), (3, [0, 1, 2]), (7, [0, 1, 2, 6]), (12, [0, 1, 2, 6, 7]), (99, [0, 1, 2, 6, 7])):
        _, _, c, p, _ = collapse_ref.collapse(keys, valid, 20, 100, doc, score, np.array([count]), 12, 1, own)
        assert c.tolist() == [len(pos)] and p[0, : len(pos)].tolist() == pos
    # group sizes are those of the live prefix
    _, _, _, _, g = collapse_ref.collapse(keys, valid, 20, 100, doc, score, np.array([7]), 12, 1, own)
    assert g[0, :4].tolist() == [3, 1, 1, 1]
    # ids below doc_base, at doc_base + n_docs and -1 are dead, and a dead position between two members does not count as earlier
    d2 = np.array([[103, 99, 120, -1, 104, 106]], dtype=np.int32)
    _, _, c, p, g = collapse_ref.collapse(keys, None, 20, 100, d2, np.zeros((1, 6), np.float32), None, 6, 2, own)
    assert c.tolist() == [2] and p[0, :2].tolist() == [0, 4] and g[0, :2].tolist() == [3, 3]
    # no validity row: the docs 10 and 11 carry their stored 7 and join group A
    _, _, c, p, g = collapse_ref.collapse(keys, None, 20, 100, doc, score, None, 12, 1, own)
    assert p[0, : c[0]].tolist() == [0, 1, 6] and g[0, :3].tolist() == [6, 3, 2]


@pytest.mark.parametrize("policy", ["own", "one", "drop"])
def test_collapsing_a_collapsed_prefix(policy):
    """collapse(collapse(A) ++ B) == collapse(A ++ B) when A was not cut at k: what lets the paged door keep only its survivors"""
    pol = collapse_ref.POLICY[policy]
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n_docs = 40
        keys = rng.integers(0, 5, n_docs).astype(np.int64)
        valid = rng.random(n_docs) > 0.2
        docs = rng.permutation(n_docs + 6) - 3  # a few ids outside the table on both sides
        la, lb = int(rng.integers(1, 25)), int(rng.integers(1, 20))
        a, b = docs[:la].astype(np.int32)[None], docs[la: la + lb].astype(np.int32)[None]
        sa, sb = rng.standard_normal((1, la)).astype(np.float32), rng.standard_normal((1, lb)).astype(np.float32)
        per_group, k = int(rng.integers(1, 4)), int(rng.integers(1, la + lb + 1))
        ad, as_, _, _, _ = collapse_ref.collapse(keys, valid, n_docs, 0, a, sa, None, la, per_group, pol)  # uncut: k = its length
        got = collapse_ref.collapse(keys, valid, n_docs, 0, np.concatenate([ad, b], 1), np.concatenate([as_, sb], 1), None, k, per_group, pol)
        want = collapse_ref.collapse(keys, valid, n_docs, 0, np.concatenate([a, b], 1), np.concatenate([sa, sb], 1), None, k, per_group, pol)
        for x, y in zip(got[:3], want[:3]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), seed


# ---- collapse_deep over a fake search ----------------------------------------------------------------------------------------------
class _FakeSearch:
    """Rankings on CPU tensors: query q's complete ranking is ``rankings[q]`` = (docs, scores), scores strictly descending.  A call
    returns the next kk rows ranked strictly after the bound row; a bound of score 0 has nothing after it."""

    def __init__(self, rankings):
        self.rankings, self.calls = rankings, []

    def __call__(self, q_ptr, q_term, q_weight, kk, after=None):
        self.calls.append((int(kk), after is not None))
        nq = len(self.rankings)
        d, s, c = torch.full((nq, kk), -1, dtype=torch.int32), torch.zeros((nq, kk), dtype=torch.float32), torch.zeros(nq, dtype=torch.int32)
        for q, (docs, scores) in enumerate(self.rankings):
            start = 0 if after is None else int(np.searchsorted(-scores, -float(after[1][q]), side="right"))
            if after is not None:
                assert after[0].dtype == torch.int32 and after[1].dtype == torch.float32
                assert float(after[1][q]) == 0.0 or int(docs[start - 1]) == int(after[0][q])  # the bound is a row of the ranking
            n = min(kk, len(docs) - start)
            d[q, :n], s[q, :n], c[q] = torch.from_numpy(docs[start: start + n]), torch.from_numpy(scores[start: start + n]), n
        return d, s, c


def _ref_collapse_fn(keys, per_group, policy, seen):
    def fn(d, s, c, kk):
        seen.append(int(d.shape[1]))
        out = collapse_ref.collapse(keys, None, len(keys), 0, d.numpy(), s.numpy(), None if c is None else c.numpy(), kk, per_group, policy)
        return tuple(torch.from_numpy(x) for x in out[:3])
    return fn


def _deep_case():
    n = 3000
    rng = np.random.default_rng(5)
    docs = rng.permutation(n).astype(np.int32)
    scores = np.linspace(30.0, 1.0, n).astype(np.float32)
    keys = np.arange(10_000, 10_000 + n, dtype=np.int64)  # distinct ...
    keys[docs[:2500]] = 42                                   # ... but the ranks 1..2500 share one key
    short = (docs[:100].copy(), scores[:100].copy())         # a second query whose ranking has 100 rows, all of the one group
    return n, keys, [(docs, scores), short]


def _whole(keys, ranking, k, per_group):
    rows = collapse_ref.collapse_list([int(x) for x in keys], None, len(keys), 0, ranking[0], ranking[1].view(np.uint32), None, k, per_group,
                                      collapse_ref.NULL_OWN)
    return [r[0] for r in rows], [r[1] for r in rows]


@pytest.mark.parametrize("per_group", [1, 3])
def test_collapse_deep_pages_until_k_groups(per_group):
    n, keys, rankings = _deep_case()
    q_ptr = torch.zeros(3, dtype=torch.int32)
    fake, seen = _FakeSearch(rankings), []
    d, s, c = collapse_deep(fake, _ref_collapse_fn(keys, per_group, collapse_ref.NULL_OWN, seen), q_ptr, None, None, 5, 64, page=1024)
    # ranks 1..2500 are one group: 64 + 1024 + 1024 rows end at rank 2112, the third page brings the other groups
    assert fake.calls == [(64, False), (1024, True), (1024, True), (1024, True)]
    assert seen == [64, 5 + 1024, 5 + 1024, 5 + 1024] and max(seen) <= collapse_ref.MAX_M
    for q, ranking in enumerate(rankings):
        docs, bits = _whole(keys, ranking, 5, per_group)
        assert int(c[q]) == len(docs) and d[q, : len(docs)].tolist() == docs and s[q].numpy().view(np.uint32)[: len(docs)].tolist() == bits
        assert d[q, len(docs):].tolist() == [-1] * (5 - len(docs))
    assert int(c[0]) == 5 and int(c[1]) == per_group  # the exhausted ranking returns short


def test_collapse_deep_exhausted_and_max_depth():
    n, keys, rankings = _deep_case()
    q_ptr2, q_ptr1 = torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    own = collapse_ref.NULL_OWN
    # only the short ranking: its second page comes back short, and that ends the loop
    fake = _FakeSearch(rankings[1:])
    d, s, c = collapse_deep(fake, _ref_collapse_fn(keys, 1, own, []), q_ptr1, None, None, 5, 64)
    assert fake.calls == [(64, False), (1024, True)] and c.tolist() == [1] and d[0].tolist() == [int(rankings[1][0][0]), -1, -1, -1, -1]
    # a ranking shorter than the first fetch: one call
    fake = _FakeSearch([(rankings[0][0][:40].copy(), rankings[0][1][:40].copy())])
    d, s, c = collapse_deep(fake, _ref_collapse_fn(keys, 1, own, []), q_ptr1, None, None, 5, 64)
    assert fake.calls == [(64, False)] and c.tolist() == [1]
    # max_depth stops early and returns what the rows read so far hold -- fewer than k, not an error
    for depth, calls in ((1088, [(64, False), (1024, True)]), (1500, [(64, False), (1024, True), (412, True)]), (32, [(32, False)]), (3, [(3, False)])):
        fake = _FakeSearch(rankings)
        d, s, c = collapse_deep(fake, _ref_collapse_fn(keys, 1, own, []), q_ptr2, None, None, 5, 64, max_depth=depth)
        assert fake.calls == calls and c.tolist() == [1, 1] and d.shape == (2, 5)
    # deep enough: the same rows as without a limit
    fake = _FakeSearch(rankings)
    d, s, c = collapse_deep(fake, _ref_collapse_fn(keys, 1, own, []), q_ptr2, None, None, 5, 64, max_depth=2600)
    assert fake.calls[-1] == (2600 - 2112, True) and d[0].tolist() == _whole(keys, rankings[0], 5, 1)[0]
    # every query done after the first fetch: no page
    fake = _FakeSearch(rankings)
    d, s, c = collapse_deep(fake, _ref_collapse_fn(np.arange(n, dtype=np.int64), 1, own, []), q_ptr2, None, None, 5, 64)
    assert fake.calls == [(64, False)] and c.tolist() == [5, 5]


def test_pool_depth():
    assert collapse_pool_depth(10, None, 10 ** 6) == 100 and collapse_pool_depth(50, None, 10 ** 6) == 200
    assert collapse_pool_depth(500, None, 10 ** 6) == 1024 and collapse_pool_depth(10, None, 30) == 30 and collapse_pool_depth(10, 7, 30) == 7
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="collapse_pool"):
            collapse_pool_depth(10, bad, 100)


# ---- the Python doors before any device ------------------------------------------------------------------------------------------
def _cpu_table():
    n = 8
    cols = fields.host_columns({"parent": np.arange(n, dtype=np.int64), "year": np.arange(n, dtype=np.int32), "flag": np.arange(n) % 2 == 0,
                                "src": ["a", "b", None, "a", "b", "a", "b", "c"], "price": np.ones(n, np.float32), "tags": [["x"], ["y"]] * 4})
    tensors = {name: (torch.from_numpy(c.data), None) for name, c in cols.items()}
    return fields.FieldTable(cols, tensors, torch.device("cpu"))


def test_field_table_refusals():
    t = _cpu_table()
    doc, score = torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.float32)
    for door in (t.collapse_device, t.collapse):
        args = (doc, score, None, 2) if door is t.collapse_device else (doc.numpy(), score.numpy(), None, 2)
        with pytest.raises(ValueError, match="unknown field 'nope'"):
            door("nope", *args)
        with pytest.raises(ValueError, match="'price' is a float column"):
            door("price", *args)
        with pytest.raises(ValueError, match="'tags' is a set column"):
            door("tags", *args)
        for bad in (0, -1, 2 ** 31, 1.5, True):
            with pytest.raises(ValueError, match="per_group"):
                door("parent", *args, per_group=bad)
        with pytest.raises(ValueError, match="nulls must be one of own, one, drop"):
            door("parent", *args, nulls="keep")
    deep_d, deep_s = torch.zeros((1, 2049), dtype=torch.int32), torch.zeros((1, 2049), dtype=torch.float32)
    with pytest.raises(ValueError, match="2048"):
        t.collapse_device("src", deep_d, deep_s, None, 5)
    with pytest.raises(ValueError, match="2048"):
        t.collapse("year", deep_d.numpy(), deep_s.numpy(), None, 5)
    with pytest.raises(ValueError, match="int32 tensor"):
        t.collapse_device("parent", doc.long(), score, None, 2)
    with pytest.raises(ValueError, match="float32 tensor of doc's shape"):
        t.collapse_device("parent", doc, score[:, :3], None, 2)
    with pytest.raises(ValueError, match=r"count must be an int32 tensor \[nq\]"):
        t.collapse_device("parent", doc, score, torch.zeros(3, dtype=torch.int32), 2)
    for k in (0, 5):
        with pytest.raises(ValueError, match="k must be in"):
            t.collapse_device("flag", doc, score, None, k)
    for name, moved in (("doc", (doc.to("meta"), score, None)), ("score", (doc, score.to("meta"), None)),
                        ("count", (doc, score, torch.zeros(2, dtype=torch.int32, device="meta")))):
        with pytest.raises(ValueError, match=f"{name} is on meta"):
            t.collapse_device("parent", *moved, 2)
    with pytest.raises(ValueError, match="score must have doc's shape"):
        t.collapse("parent", doc.numpy(), score.numpy()[:, :2], None, 2)


@pytest.fixture()
def one_rank_group():
    import torch.distributed as dist
    assert not dist.is_initialized()
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", init_method=f"file://{os.path.join(tmp, 'rendezvous')}", rank=0, world_size=1)
        try:
            yield
        finally:
            dist.destroy_process_group()


def test_mirrors_unchanged_without_keyword_and_refusals(golden_dir, one_rank_group, tmp_path):
    """The fake backend of test_dict_search_cpu.py (the CPU oracle behind the sharding protocol, counting its searches): a call
    without ``collapse_by`` searches and caches as before; with it, a backend without fields, a bad column, a ``top_k`` above 1 024
    and a sharded backend refuse before they search."""
    from test_dict_search_cpu import _Counted
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    q = {qid: j["queries"][qid] for qid in ("q0", "q1", "q2")}
    n = len(j["corpus"])
    for make, method in ((lambda f: sparse_rx.RetrievalService(shard_searcher_factory=f, sharded=True), "search_bm25"),
                         (lambda f: sparse_rx.OptimizedBM25Retriever(shard_searcher_factory=f, sharded=True), "search"),
                         (lambda f: sparse_rx.OptimizedRetriever({"type": "bm25"}, shard_searcher_factory=f, sharded=True, cache_dir=str(tmp_path)), "search")):
        f = _Counted()
        o = make(f)
        (o.build_bm25_index if method == "search_bm25" else o.build_index_from_corpus)(j["corpus"])
        search = getattr(o, method)
        r = search(q, top_k=10)
        assert f.take() == [(3, 10)] and len(o.query_cache) == 3 and all(r[qid] for qid in q)
        # the keywords at their defaults: the same dicts, from the cache
        assert search(q, top_k=10, collapse_by=None) == r and search(q, top_k=10, collapse_by=None, per_group=0, collapse_nulls="zz") == r
        assert f.take() == []
        with pytest.raises(ValueError, match=rf"{method}\(collapse_by=\.\.\.\) needs the docs' fields: call set_doc_fields"):
            search(q, top_k=10, collapse_by="parent")
        o.set_doc_fields({"parent": np.arange(n, dtype=np.int64) // 4, "price": np.ones(n, np.float32), "tags": [["x"]] * n,
                          "src": ["s%d" % (i % 3) for i in range(n)]})
        assert search(q, top_k=10) == r and f.take() == []
        with pytest.raises(ValueError, match="unknown field 'nope'"):
            search(q, top_k=10, collapse_by="nope")
        with pytest.raises(ValueError, match="'price' is a float column"):
            search(q, top_k=10, collapse_by="price")
        with pytest.raises(ValueError, match="'tags' is a set column"):
            search(q, top_k=10, collapse_by="tags")
        with pytest.raises(ValueError, match="at most 1024 rows per query, got top_k=1025"):
            search(q, top_k=1025, collapse_by="parent")
        with pytest.raises(ValueError, match="per_group"):
            search(q, top_k=10, collapse_by="parent", per_group=0)
        with pytest.raises(ValueError, match="nulls must be"):
            search(q, top_k=10, collapse_by="parent", collapse_nulls="zz")
        with pytest.raises(ValueError, match="collapse_depth must be >= 1"):
            search(q, top_k=10, collapse_by="parent", collapse_depth=0)
        for kw in (dict(collapse_by="parent"), dict(collapse_by="src", per_group=2), dict(collapse_by="parent", excluded_docs=[next(iter(j["corpus"]))])):
            with pytest.raises(ValueError, match="whole index on one GPU"):
                search(q, top_k=10, **kw)
        if method == "search_bm25":
            with pytest.raises(ValueError, match="'price' is a float column"):
                o.collapse(r, "price")
            with pytest.raises(ValueError, match="whole index on one GPU"):
                o.collapse(r, "parent")
        assert f.take() == [] and len(o.query_cache) == 3
        o.close()


def test_service_doors_before_any_device():
    svc = sparse_rx.RetrievalService(device="cuda:0")
    with pytest.raises(ValueError, match=r"collapse\(\.\.\.\) needs the docs' fields: call set_doc_fields"):
        svc.collapse({"q": {"d0": 1.0}}, "parent")
    with pytest.raises(ValueError, match="not built"):
        svc.search_bm25({"q": "w"}, collapse_by="parent")
    for cls in (sparse_rx.HybridRetriever, sparse_rx.ShardedSearcher, sparse_rx.HostBatchPipeline):
        assert not hasattr(cls, "collapse")
        for name in ("search", "submit"):
            if hasattr(cls, name):
                assert "collapse_by" not in inspect.signature(getattr(cls, name)).parameters
    defaults = dict(collapse_by=None, per_group=1, collapse_nulls="own", collapse_depth=None)
    for fn in (sparse_rx.RetrievalService.search_bm25, sparse_rx.OptimizedBM25Retriever.search, sparse_rx.OptimizedRetriever.search):
        for name, default in defaults.items():
            p = inspect.signature(fn).parameters[name]
            assert p.default == default and p.kind is inspect.Parameter.KEYWORD_ONLY
    for name, default in dict(collapse_by=None, per_group=1, collapse_nulls="own", collapse_pool=None).items():
        p = inspect.signature(sparse_rx.RetrievalService.search_hybrid).parameters[name]
        assert p.default == default and p.kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(sparse_rx.RetrievalService.collapse).parameters
    assert [sig[n].default for n in ("top_k", "per_group", "nulls")] == [10, 1, "own"]
    spec = CollapseSpec("parent")
    assert (spec.by, spec.per_group, spec.nulls, spec.depth) == ("parent", 1, "own", None)
