"""Term constraints without a GPU: the seventh header and its symbol table, every refusal of the two entry points (none reaches
a device), the NumPy restatement (tests/terms_ref.py) on an example worked by hand, the keyword resolution of the API mirrors
(term_filter_spec, parse_operators, the combination with doc filters) and the mirrors with no keyword given."""
import ctypes
import os
import re
import tempfile

import numpy as np
import pytest

import filter_ref
import terms_ref
import sparse_rx
from sparse_rx import _capi
from sparse_rx.backend import TermFilterSpec, apply_operators, doc_filter_spec, term_filter_spec
from sparse_rx.index import parse_operators, term_lists_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(12)]  # 16-byte aligned addresses, never dereferenced


def test_seventh_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "sparse_rx_terms.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_capi.TERMS_SYMBOLS) and len(declared) == 2, declared ^ set(_capi.TERMS_SYMBOLS)
    assert '#include "sparse_rx_filter.h"' in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS, _capi.MMR_SYMBOLS)
    assert [len(t) for t in others] == [35, 4, 4, 8, 5, 3]
    for other in others:
        assert not set(_capi.TERMS_SYMBOLS) & set(other)
    assert "terms.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "sparse_rx_terms.h") in _capi._deps()
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.TERMS_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert sparse_rx.parse_operators is parse_operators


def _refused(rc, word):
    msg = _capi.lib().srx_last_error()
    assert rc == -1 and word.encode() in msg, (rc, msg)


def test_bytes_call():
    f = _capi.lib().srx_filter_from_terms_bytes
    assert f(0, 100) == 0 and f(1, 1) == 16 and f(3, 100) == 3 * 4 * 4 and f(1000, 20_011) == 1000 * 628 * 4
    assert f(7, 2 ** 31 - 2) == 7 * 67_108_864 * 4
    for n_rows, n_docs in ((-1, 100), (1, 0), (1, -5), (1, 2 ** 31 - 1), (1, 2 ** 40)):
        _refused(f(n_rows, n_docs), "srx_filter_from_terms_bytes")
    _refused(f(2 ** 62, 100), "does not fit int64")


def _desc(**kw):
    d = dict(device=0, val_type=0, n_docs=1000, vocab=50, nnz=4000, n_blocks=2000, doc_base=0, tile_log2=6, n_tiles=16, unit_tiles=1,
             term_ptr=P[0], post=P[1], tile_skip=P[2], idf=P[3], term_bound=None, post16=P[4])
    d.update(kw)
    return ctypes.byref(_capi.IndexDesc(**d))


def _base(**kw):
    d = dict(bits=P[8], n_filters=1, q_filter=None)
    d.update(kw)
    return ctypes.byref(_capi.DocFilterDesc(**d))


def test_builder_refusals():
    L = _capi.lib()
    ok = dict(desc=_desc(), n_rows=3, all_ptr=P[5], all_term=P[6], any_ptr=None, any_term=None, none_ptr=P[7], none_term=P[9], base=None,
              out=P[10], stream=None)
    call = lambda **kw: L.srx_filter_from_terms(*{**ok, **kw}.values())
    # the descriptor, as srx_score_docs refuses it
    _refused(call(desc=None), "null descriptor")
    _refused(call(desc=_desc(val_type=2)), "bad val_type")
    for kw in (dict(n_docs=0), dict(n_docs=2 ** 31 - 1), dict(vocab=0)):
        _refused(call(desc=_desc(**kw)), "n_docs / vocab out of range")
    for t in (5, 15):
        _refused(call(desc=_desc(tile_log2=t)), "tile_log2 must be in [6, 14]")
    _refused(call(desc=_desc(n_tiles=15)), "n_tiles != ceil")
    for u in (0, 65):
        _refused(call(desc=_desc(unit_tiles=u)), "unit_tiles must be in [1, 64]")
    _refused(call(desc=_desc(post=None, post16=None)), "neither post nor post16")
    _refused(call(desc=_desc(n_docs=70_000, tile_log2=14, n_tiles=5, unit_tiles=4)), "units of <= 49152 docs")
    for null in ("term_ptr", "tile_skip", "idf"):
        _refused(call(desc=_desc(**{null: None})), "null term_ptr / tile_skip / idf")
    # the call's own arguments
    _refused(call(n_rows=-1), "n_rows < 0")
    for half in ("all_ptr", "all_term", "none_ptr", "none_term"):
        _refused(call(**{half: None}), "go together")
    _refused(call(any_ptr=P[5]), "go together")
    _refused(call(any_term=P[5]), "go together")
    _refused(call(out=None), "null out_bits")
    for off in (4, 8, 2):
        _refused(call(out=P[10] + off), "16-byte aligned")
    # the base, by the filter header's rules
    _refused(call(base=_base(bits=None)), "null filter bits")
    _refused(call(base=_base(bits=P[8] + 4)), "16-byte aligned")
    for nf in (0, -1):
        _refused(call(base=_base(n_filters=nf)), "n_filters")
    assert b"srx_filter_from_terms" in L.srx_last_error()
    # nothing to do: no launch, with or without lists and base
    assert call(n_rows=0) == 0
    assert call(n_rows=0, base=_base(), all_ptr=None, all_term=None, none_ptr=None, none_term=None) == 0
    _refused(call(n_rows=0, out=None), "null out_bits")  # the checks come first


# ---- the restatement on an example worked by hand ------------------------------------------------------------------------------
def _hand_corpus():
    """40 docs, 4 terms: term 0 in the even docs, term 1 in the multiples of 3, term 2 in docs 31..39, term 3 in no doc; doc 6 lists
    term 0 twice (one posting)."""
    docs = []
    for d in range(40):
        row = ([0] if d % 2 == 0 else []) + ([1] if d % 3 == 0 else []) + ([2] if d >= 31 else [])
        if d == 6:
            row = [0, 0, 1]
        docs.append(row)
    indptr = np.cumsum([0] + [len(r) for r in docs])
    indices = np.asarray([t for r in docs for t in r], dtype=np.int32)
    return indptr, indices


def test_restatement_by_hand():
    indptr, indices = _hand_corpus()
    n = 40
    terms_ref.assert_no_stored_zero(np.ones(len(indices), np.float32))
    with pytest.raises(AssertionError):
        terms_ref.assert_no_stored_zero(np.asarray([1.0, 0.0]))
    even, third, late = np.arange(n) % 2 == 0, np.arange(n) % 3 == 0, np.arange(n) >= 31
    assert np.array_equal(terms_ref.docs_with_term(indptr, indices, n, 0), even)
    assert not terms_ref.docs_with_term(indptr, indices, n, 3).any() and not terms_ref.docs_with_term(indptr, indices, n, -1).any()
    all_ = [[0], [0, 1], [], [], [], [-1], [0], [], [0], [0, 0, 1]]
    any_ = [[], [], [1, 2], [], [], [], [-1], [-1, 2], [], [2, 2]]
    none = [[], [], [], [0], [], [], [], [-1], [0], [3, -1]]
    m = terms_ref.term_masks(indptr, indices, n, all_, any_, none)
    assert m.shape == (10, n)
    assert np.array_equal(m[0], even) and np.array_equal(m[1], even & third) and np.array_equal(m[2], third | late)
    assert np.array_equal(m[3], ~even)
    assert m[4].all()                                # the empty triple: every doc
    assert not m[5].any()                            # -1 in all: no doc
    assert not m[6].any()                            # -1 alone in any: the list is not empty, and no doc has one of its terms
    assert np.array_equal(m[7], late)                # -1 next to a real term in any contributes nothing; -1 in none has no effect
    assert not m[8].any()                            # a term in all and in none
    assert np.flatnonzero(m[9]).tolist() == [36]     # duplicates: even, multiple of 3, >= 31
    assert np.flatnonzero(m[1]).tolist() == [0, 6, 12, 18, 24, 30, 36]
    # packed as a filter row: 40 docs are 2 words, padded to 4
    assert filter_ref.pack(m[1]).tolist() == [sum(1 << d for d in (0, 6, 12, 18, 24, 30)), 1 << 4, 0, 0]
    assert np.array_equal(sparse_rx.filter.pack_masks(m), np.stack([filter_ref.pack(r) for r in m]))
    # with a base: q_base picks the base row of every output row, -1 none; None is row 0
    base = np.stack([np.arange(n) < 20, np.arange(n) >= 20])
    q_base = [0, 1, -1, 0, 1, 0, 0, 1, 0, -1]
    b = terms_ref.term_masks(indptr, indices, n, all_, any_, none, base, q_base)
    assert np.array_equal(b[0], even & base[0]) and np.array_equal(b[1], even & third & base[1]) and np.array_equal(b[2], m[2])
    assert np.array_equal(b[4], base[1]) and np.array_equal(b[9], m[9])
    b0 = terms_ref.term_masks(indptr, indices, n, all_, None, None, base)
    assert np.array_equal(b0[0], even & base[0]) and np.array_equal(b0[2], base[0])
    # a list that is absent altogether is an empty list in every row
    assert np.array_equal(terms_ref.term_masks(indptr, indices, n, None, None, none), np.stack([~even if r in (3, 8) else np.ones(n, bool) for r in range(10)]))


def test_term_lists_csr():
    ptr, term = term_lists_csr([[3, -1], [], [0, 0, 49]], 50, "all_terms")
    assert ptr.dtype == term.dtype == np.int32 and ptr.tolist() == [0, 2, 2, 5] and term.tolist() == [3, -1, 0, 0, 49]
    ptr, term = term_lists_csr([], 50)
    assert ptr.tolist() == [0] and term.size == 0
    for bad in ([[50]], [[-2]], [[1.5]], [3], "ab", [["a"]], [[[1]]]):
        with pytest.raises(ValueError):
            term_lists_csr(bad, 50)


# ---- the keywords of the API mirrors ---------------------------------------------------------------------------------------
VOCAB = {"gpu": 0, "accelerator": 1, "mi355x": 2, "deprecated": 3, "ünï": 4}
QUERIES = {"a": "x", "b": "y", "c": "z"}


def test_term_filter_spec():
    assert term_filter_spec(VOCAB, QUERIES) is None
    assert term_filter_spec(VOCAB, QUERIES, [], None, ()) is None  # nothing constrains a query
    s = term_filter_spec(VOCAB, QUERIES, ["MI355X", "unknown"], ["gpu accelerator"], ["deprecated"])
    assert isinstance(s, TermFilterSpec)
    assert s.rows == [((2, -1), (0, 1), (3,))]            # lower-cased; an OOV word is -1; a string of two tokens adds both
    assert s.row_of_qid == {"a": 0, "b": 0, "c": 0}
    assert term_filter_spec(VOCAB, QUERIES, ["gpu-accelerator, ÜNÏ!"]).rows == [((0, 1, 4), (), ())]
    for kw in (dict(must_terms=["  "]), dict(any_terms=["gpu", "..."]), dict(must_not_terms={"a": [""]}), dict(must_terms=[7])):
        with pytest.raises(ValueError, match="holds no token"):
            term_filter_spec(VOCAB, QUERIES, **kw)
    for kw in (dict(must_terms="gpu"), dict(any_terms=b"gpu"), dict(must_not_terms={"a": "gpu"})):
        with pytest.raises(ValueError, match="not one string"):
            term_filter_spec(VOCAB, QUERIES, **kw)
    # the dict form: a qid missing from all three is not constrained; equal triples share a row
    s = term_filter_spec(VOCAB, QUERIES, {"a": ["gpu"], "c": ["gpu"], "other": ["mi355x"]}, None, {"c": []})
    assert s.rows == [((0,), (), ())] and s.row_of_qid == {"a": 0, "b": -1, "c": 0}
    s = term_filter_spec(VOCAB, QUERIES, {"a": ["gpu"]}, ["accelerator"], {"c": ["gpu"]})
    assert s.rows == [((0,), (1,), ()), ((), (1,), ()), ((), (1,), (0,))] and s.row_of_qid == {"a": 0, "b": 1, "c": 2}
    assert term_filter_spec(VOCAB, QUERIES, {"other": ["gpu"]}) is None


def test_term_spec_with_doc_filter():
    row_of = {f"d{i}": i for i in range(10)}
    terms = term_filter_spec(VOCAB, QUERIES, {"a": ["gpu"], "b": ["gpu"]})
    assert terms.with_base(None, QUERIES) is terms
    docs = doc_filter_spec(row_of, QUERIES, {"b": ["d1"], "c": ["d2", "d3"]}, None)
    s = terms.with_base(docs, QUERIES)
    # distinct (doc row, term row) pairs: a = (-1, 0), b = (0, 0), c = (1, -1)
    assert s.base is docs and s.row_of_qid == {"a": 0, "b": 1, "c": 2}
    assert s.rows == [((0,), (), ()), ((0,), (), ()), ((), (), ())] and s.base_rows == [-1, 0, 1]
    docs = doc_filter_spec(row_of, QUERIES, None, ["d5"])  # one list for every query: a and b share (0, 0)
    s = terms.with_base(docs, QUERIES)
    assert s.row_of_qid == {"a": 0, "b": 0, "c": 1} and s.base_rows == [0, 0] and s.rows == [((0,), (), ()), ((), (), ())]
    docs = doc_filter_spec(row_of, QUERIES, {"other": ["d0"]}, None)  # filters no qid of the call
    s = term_filter_spec(VOCAB, QUERIES, {"a": ["gpu"]}).with_base(docs, QUERIES)
    assert s.row_of_qid == {"a": 0, "b": -1, "c": -1} and s.base_rows == [-1]


@pytest.mark.parametrize("text,expect", [
    ("+a -b c", ("a c", ["a"], ["b"])),
    ("a-b", ("a-b", [], [])),
    ("+ a", ("+ a", [], [])),
    ("-", ("-", [], [])),
    ("+", ("+", [], [])),
    ("", ("", [], [])),
    ("  x   +y  ", ("x y", ["y"], [])),
    ("-ünï +日本 +_x", ("日本 _x", ["日本", "_x"], ["ünï"])),
    ("--a ++b -+c +-d", ("--a ++b -+c +-d", [], [])),
    ("+a-b -c+d", ("a-b", ["a-b"], ["c+d"])),
    ("-a -a +a", ("a", ["a"], ["a", "a"])),
])
def test_parse_operators(text, expect):
    assert parse_operators(text) == expect


def test_apply_operators():
    q = {"a": "+gpu fast -old", "b": "plain", "c": "", "d": None}
    texts, must, must_not = apply_operators(q)
    assert texts == {"a": "gpu fast", "b": "plain", "c": "", "d": None}
    assert must == {"a": ["gpu"], "b": [], "c": [], "d": []} and must_not == {"a": ["old"], "b": [], "c": [], "d": []}
    texts, must, must_not = apply_operators(q, ["mi355x"], {"b": ["deprecated"], "zz": ["x"]})
    assert must == {"a": ["mi355x", "gpu"], "b": ["mi355x"], "c": ["mi355x"], "d": ["mi355x"]}
    assert must_not == {"a": ["old"], "b": ["deprecated"], "c": [], "d": []}
    for kw in (dict(must_terms="gpu"), dict(must_not_terms={"a": "gpu"})):
        with pytest.raises(ValueError, match="not one string"):
            apply_operators(q, **kw)
    # merged, the result is what the keywords alone give
    texts, must, must_not = apply_operators(q)
    s = term_filter_spec({"gpu": 0, "old": 1}, texts, must, None, must_not)
    assert s.rows == [((0,), (), (1,))] and s.row_of_qid == {"a": 0, "b": -1, "c": -1, "d": -1}


# ---- the mirrors with no keyword given, and the sharded refusal -----------------------------------------------------------------
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


def test_mirrors_unchanged_without_keywords_and_sharded_refusal(golden_dir, one_rank_group):
    """The fake backend of test_dict_search_cpu.py (the CPU oracle behind the sharding protocol, counting its searches): a call
    without the new keywords searches and caches as before; with one, a sharded backend refuses before it searches."""
    import json
    from test_dict_search_cpu import _Counted
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    q = {qid: j["queries"][qid] for qid in ("q0", "q1", "q2")}
    for make, method in ((lambda f: sparse_rx.RetrievalService(shard_searcher_factory=f, sharded=True), "search_bm25"),
                         (lambda f: sparse_rx.OptimizedBM25Retriever(shard_searcher_factory=f, sharded=True), "search")):
        f = _Counted()
        o = make(f)
        (o.build_bm25_index if method == "search_bm25" else o.build_index_from_corpus)(j["corpus"])
        search = getattr(o, method)
        r = search(q, top_k=10)
        assert f.take() == [(3, 10)] and len(o.query_cache) == 3 and all(r[qid] for qid in q)
        # every new keyword at its default, spelled out: the same dicts, served from the cache
        assert search(q, top_k=10, must_terms=None, any_terms=None, must_not_terms=None, operators=False) == r and f.take() == []
        assert search(q, top_k=10, operators=True) == r and f.take() == []  # no +word / -word in the texts: nothing is constrained
        for kw in (dict(must_terms=["w3"]), dict(any_terms={"q0": ["w3"]}), dict(must_not_terms=["w3"]), dict(must_terms=["nosuchword"])):
            with pytest.raises(ValueError, match="whole index on one GPU"):
                search(q, top_k=10, **kw)
        with pytest.raises(ValueError, match="whole index on one GPU"):
            search({"q0": q["q0"] + " -w3"}, top_k=10, operators=True)
        assert f.take() == [] and len(o.query_cache) == 3
        o.close()


def test_search_by_vector_takes_sequences_only():
    svc = sparse_rx.RetrievalService(device="cuda:0")
    for kw in ("must_terms", "any_terms", "must_not_terms"):
        with pytest.raises(ValueError, match="must be a sequence of strings"):  # checked before the index is looked at
            svc.search_by_vector(np.zeros(4, np.float32), **{kw: {"q": ["w3"]}})
