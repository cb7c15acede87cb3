"""The filter keywords of the API mirrors as ONE chain, without a GPU: ``with_base`` of the row-built specs over every pair of
kinds against a restatement, ``SparseBackend.filter_spec`` on a host-only backend against the three resolutions chained by hand,
and the list marshalling of the row builders' door (``filter.builder_lists`` / ``filter.build_rows``) on CPU tensors."""
import itertools
import types

import numpy as np
import pytest
import torch

from sparse_rx.backend import (DocFilterSpec, FieldFilterSpec, RowFilterSpec, SparseBackend, TermFilterSpec, doc_filter_spec, field_filter_spec,
                               term_filter_spec)
from sparse_rx.fields import host_columns
from sparse_rx.filter import BASE_NAMES, build_rows, builder_lists, resolve_filter
from sparse_rx.index import build_host_index

QUERIES = {"a": "x", "b": "y", "c": "z"}
ROW_OF = {f"d{i}": i for i in range(10)}
VOCAB = {"gpu": 0, "accelerator": 1, "old": 2}
SCHEMA = host_columns({"year": np.arange(2000, 2010, dtype=np.int32), "src": ["wiki", "web"] * 5})
G1 = {"must": [{"field": "year", "gte": 2005}]}
G2 = [{"field": "src", "eq": "wiki"}]
EMPTY = ((), (), ())

# per kind: a dict keyword that names some qids, a shared keyword, a keyword that names no qid of the call
KIND = {
    "doc": {"some": lambda: doc_filter_spec(ROW_OF, QUERIES, {"b": ["d1"], "c": ["d2", "d3"]}, None),
            "shared": lambda: doc_filter_spec(ROW_OF, QUERIES, None, ["d5"]),
            "none": lambda: doc_filter_spec(ROW_OF, QUERIES, {"other": ["d0"]}, None)},
    "term": {"some": lambda: term_filter_spec(VOCAB, QUERIES, {"a": ["gpu"], "b": ["gpu"]}),
             "shared": lambda: term_filter_spec(VOCAB, QUERIES, None, ["accelerator"]),
             "none": lambda: term_filter_spec(VOCAB, QUERIES, {"other": ["gpu"]})},
    "field": {"some": lambda: field_filter_spec(SCHEMA, QUERIES, {"a": G1, "b": G1, "c": {"must": G1["must"], "must_not": G2}}),
              "shared": lambda: field_filter_spec(SCHEMA, QUERIES, G2),
              "none": lambda: field_filter_spec(SCHEMA, QUERIES, {"other": G1})},
}
CHAINS = [("doc", "term"), ("doc", "field"), ("term", "field"), ("doc", "term", "field")]


def chain(specs, queries):
    """The kinds' specs (None: the kind constrains no query) chained as the backend chains them"""
    spec = None
    for s in specs:
        if s is not None:
            spec = s.with_base(spec, queries) if isinstance(s, RowFilterSpec) else s
    return spec


def restated(specs, queries):
    """(rows, row_of_qid, base_rows) of the chained spec.  Per qid the tuple of its rows per kind; the distinct tuples numbered in
    the order of their first appearance, the all -1 tuple is -1; a row's own triple is the last kind's (none: the empty triple),
    its base row the number of the tuple without its last entry."""
    specs = [s for s in specs if s is not None]

    def numbered(kinds):
        seen, of_qid = {}, {}
        for qid in queries:
            t = tuple(s.row_of_qid[qid] for s in kinds)
            of_qid[qid] = -1 if set(t) == {-1} else seen.setdefault(t, len(seen))
        return seen, of_qid

    seen, of_qid = numbered(specs)
    if len(specs) == 1:
        return getattr(specs[0], "rows", None), of_qid, None  # a doc spec has lists, not rows
    before, _ = numbered(specs[:-1])
    rows = [specs[-1].rows[t[-1]] if t[-1] >= 0 else EMPTY for t in seen] or [EMPTY]
    base_rows = [-1 if set(t[:-1]) == {-1} else before[t[:-1]] for t in seen] or [-1]
    return rows, of_qid, base_rows


def _cases():
    for kinds in CHAINS:
        for how in itertools.product(("some", "shared", "none"), repeat=len(kinds)):
            yield pytest.param(kinds, how, id="->".join(f"{k}:{h}" for k, h in zip(kinds, how)))


@pytest.mark.parametrize("kinds,how", _cases())
def test_with_base_over_every_pair_of_kinds(kinds, how):
    specs = [KIND[k][h]() for k, h in zip(kinds, how)]
    got = chain(specs, QUERIES)
    given = [s for s in specs if s is not None]
    if not given:
        assert got is None
        return
    rows, row_of_qid, base_rows = restated(specs, QUERIES)
    assert type(got) is type(given[-1]) and got.row_of_qid == row_of_qid
    if isinstance(got, DocFilterSpec):  # only the doc keyword constrains: the doc spec itself
        assert got is given[-1] and len(given) == 1
        return
    assert got.rows == rows and got.base_rows == base_rows
    if len(given) == 1:
        assert got is given[0] and got.base is None
    else:
        # the base is the chain of the kinds before, itself equal to its restatement
        b_rows, b_of_qid, b_base_rows = restated(given[:-1], QUERIES)
        assert got.base.row_of_qid == b_of_qid
        if isinstance(got.base, RowFilterSpec):
            assert got.base.rows == b_rows and got.base.base_rows == b_base_rows
        assert got is not given[-1] and given[-1].base is None  # with_base leaves the spec it is called on alone
    if isinstance(got, FieldFilterSpec):
        assert got.resolver is given[-1].resolver and got.table is None
    if isinstance(got, TermFilterSpec):
        assert got.sparse is None


def test_restatement_gives_the_pinned_values():
    """The values test_term_spec_with_doc_filter and test_field_spec_with_doc_and_term_bases assert, out of the restatement"""
    terms, docs = KIND["term"]["some"](), KIND["doc"]["some"]()
    assert restated([docs, terms], QUERIES) == ([((0,), (), ()), ((0,), (), ()), EMPTY], {"a": 0, "b": 1, "c": 2}, [-1, 0, 1])
    assert restated([KIND["doc"]["shared"](), terms], QUERIES) == ([((0,), (), ()), EMPTY], {"a": 0, "b": 0, "c": 1}, [0, 0])
    one = term_filter_spec(VOCAB, QUERIES, {"a": ["gpu"]})
    assert restated([KIND["doc"]["none"](), one], QUERIES) == ([((0,), (), ())], {"a": 0, "b": -1, "c": -1}, [-1])
    flds = field_filter_spec(SCHEMA, QUERIES, {"a": G1, "b": G1})
    assert restated([docs, flds], QUERIES) == ([((0,), (), ()), ((0,), (), ()), EMPTY], {"a": 0, "b": 1, "c": 2}, [-1, 0, 1])
    terms = term_filter_spec({"gpu": 0}, QUERIES, {"a": ["gpu"], "c": ["gpu"]})
    assert restated([KIND["doc"]["shared"](), terms, flds], QUERIES) == ([((0,), (), ()), ((0,), (), ()), EMPTY], {"a": 0, "b": 1, "c": 2}, [0, 1, 0])


# ---- SparseBackend.filter_spec on a host-only backend -------------------------------------------------------------------------------
CORPUS = {f"d{i}": {"text": " ".join(w for j, w in enumerate(("gpu", "accelerator", "old", "fast")) if (i >> j) & 1) or "plain"} for i in range(10)}
KEYWORDS = dict(allowed_docs={"a": ["d1", "d2"]}, excluded_docs=["d5"], must_terms={"a": ["gpu"], "b": ["gpu"]}, any_terms=["accelerator"],
                must_not_terms={"c": ["old"]}, where={"a": G1, "c": G2})


@pytest.fixture(scope="module")
def backend():
    be = SparseBackend("cuda:0", 6)
    be.set_host(build_host_index(CORPUS))  # no upload: nothing here touches a device
    be.set_fields({"year": np.arange(2000, 2010, dtype=np.int32), "src": ["wiki", "web"] * 5})
    return be


def _by_hand(be, queries, allowed_docs=None, excluded_docs=None, must_terms=None, any_terms=None, must_not_terms=None, where=None):
    """The three resolutions, chained by hand"""
    spec = doc_filter_spec({d: i for i, d in enumerate(be.host.doc_ids)}, queries, allowed_docs, excluded_docs)
    terms = term_filter_spec(be.host.vocabulary, queries, must_terms, any_terms, must_not_terms)
    if terms is not None:
        spec = terms.with_base(spec, queries)
    flds = None if where is None else field_filter_spec(be._fields, queries, where)
    if flds is not None:
        spec = flds.with_base(spec, queries)
    return spec


def _assert_same(got, exp):
    assert type(got) is type(exp)
    if exp is None:
        return
    assert got.row_of_qid == exp.row_of_qid
    if isinstance(exp, DocFilterSpec):
        assert got.allow == exp.allow and [x.tolist() for x in got.lists] == [x.tolist() for x in exp.lists]
        return
    assert got.rows == exp.rows and got.base_rows == exp.base_rows
    _assert_same(got.base, exp.base)


@pytest.mark.parametrize("names", [c for n in range(7) for c in itertools.combinations(KEYWORDS, n)], ids=lambda c: "+".join(c) or "nothing")
def test_backend_filter_spec_is_the_chain_by_hand(backend, names):
    kw = {k: KEYWORDS[k] for k in names}
    if "allowed_docs" in kw and "excluded_docs" in kw:
        with pytest.raises(ValueError, match="not both"):
            backend.filter_spec(QUERIES, **kw)
        with pytest.raises(ValueError, match="not both"):
            _by_hand(backend, QUERIES, **kw)
        return
    got = backend.filter_spec(QUERIES, **kw, call="search_x")
    _assert_same(got, _by_hand(backend, QUERIES, **kw))
    assert (got is None) == (not names)
    # what the backend binds: the term rows to its device index, the field rows to its table
    s = got
    while isinstance(s, RowFilterSpec):
        if isinstance(s, TermFilterSpec):
            assert s.sparse() is backend.dev
        else:
            assert s.table == backend.field_table
        s = s.base
    assert backend.filter_spec(QUERIES, **{k: None for k in KEYWORDS}) is None


def test_backend_filter_spec_reports_the_earlier_keyword_first(backend):
    bad = dict(allowed_docs=["nope"], must_terms="gpu", where=7)
    msg = dict(allowed_docs="unknown doc id 'nope'", must_terms="must_terms must be a sequence of strings", where="where must be a group")
    order = list(bad)
    for i, first in enumerate(order):
        for n in range(1, len(order) - i + 1):  # `first` bad, alone and with later bad keywords: its message
            with pytest.raises(ValueError, match=msg[first]):
                backend.filter_spec(QUERIES, **{k: bad[k] for k in order[i:i + n]})
    with pytest.raises(ValueError, match=msg["where"]):  # good earlier keywords: the later bad one is still reported
        backend.filter_spec(QUERIES, excluded_docs=["d5"], must_terms=["gpu"], where=7)
    with pytest.raises(ValueError, match=msg["must_terms"]):
        backend.filter_spec(QUERIES, excluded_docs=["d5"], must_terms="gpu", where=G1)
    bare = SparseBackend("cuda:0", 6)
    with pytest.raises(ValueError, match="term constraints need the sparse index: build it first"):
        bare.filter_spec(QUERIES, must_terms=["gpu"], where=G1)
    bare.set_host(build_host_index(CORPUS))
    with pytest.raises(ValueError, match=r"search_x\(where=\.\.\.\) needs the docs' fields: call set_doc_fields\(\) first"):
        bare.filter_spec(QUERIES, must_terms=["gpu"], where=G1, call="search_x")
    # one table of doc rows behind the filter path and candidate_block
    bare.filter_spec(QUERIES, allowed_docs=["d1"])
    rows = bare._rows
    bare.candidate_block(QUERIES, {"a": ["d2"]})
    assert bare._rows is rows and rows.ids is bare.host.doc_ids


# ---- the list marshalling of the row builders' door, on CPU tensors -----------------------------------------------------------------
CPU = torch.device("cpu")


def _i32(*x):
    return torch.tensor(x, dtype=torch.int32)


def test_builder_lists():
    ptr, ids = _i32(0, 2, 2), _i32(4, 7)
    n_rows, t = builder_lists(CPU, ((ptr, ids), None, (_i32(0, 0, 0), _i32())), "term")
    assert n_rows == 2 and t[2] is None and t[3] is None
    assert t[0].data_ptr() == ptr.data_ptr() and t[1].data_ptr() == ids.data_ptr() and t[4].tolist() == [0, 0, 0]
    hold = t[5]  # the empty id tensor goes as a one-element placeholder: the entry points take "ptr and ids, both or neither"
    assert hold.dtype == torch.int32 and hold.numel() == 1 and hold.dim() == 1 and hold.device == CPU and hold.is_contiguous() and hold.data_ptr() != 0
    for word in ("term", "clause"):
        for bad in ((torch.tensor([0, 1]), _i32(3)), (_i32(0, 1), torch.tensor([3.0])), (_i32(0, 1).reshape(1, 2), _i32(3)), (_i32(0, 1), _i32(3).reshape(1, 1)),
                    ([0, 1], _i32(3))):  # a wrong dtype, a 2-D tensor, not a tensor
            with pytest.raises(ValueError, match=rf"any must be a \(ptr, {word}\) pair of 1-D int32 tensors on cpu"):
                builder_lists(CPU, (None, bad, None), word)
        with pytest.raises(ValueError, match=f"the {word} lists must have one ptr entry per output row, plus one, and agree on the row count"):
            builder_lists(CPU, ((_i32(0, 1), _i32(3)), (_i32(0, 1, 1), _i32(3)), None), word)
        with pytest.raises(ValueError, match="agree on the row count"):
            builder_lists(CPU, ((_i32(), _i32()), None, None), word)
        with pytest.raises(ValueError, match="give at least one of all / any / none"):
            builder_lists(CPU, (None, None, None), word)
        with pytest.raises(ValueError, match="a filter needs at least one row"):
            builder_lists(CPU, ((_i32(0), _i32()), None, None), word)


def test_build_rows_refuses_before_it_launches():
    owner = types.SimpleNamespace(device=CPU, n_docs=100, doc_base=0)

    def launch(*args):
        raise AssertionError("launched")
    lists = ((_i32(0, 1), _i32(3)), None, None)
    with pytest.raises(ValueError, match="q_base picks rows of a base filter: it needs base="):
        build_rows(owner, "srx_filter_from_terms", launch, lists, "term", None, _i32(0), None)
    with pytest.raises(ValueError, match="base must be a DocFilter"):
        build_rows(owner, "srx_filter_from_terms", launch, lists, "term", object(), None, None)
    with pytest.raises(ValueError, match="give at least one"):  # the lists are looked at first
        build_rows(owner, "srx_filter_from_fields", launch, (None, None, None), "clause", None, _i32(0), None)
    assert resolve_filter(owner, None, None, 1, BASE_NAMES) == (None, None)
    with pytest.raises(ValueError, match="q_filter picks rows of a filter: it needs filter="):
        resolve_filter(owner, None, _i32(0), 1)
    with pytest.raises(ValueError, match="filter must be a DocFilter"):
        resolve_filter(owner, object(), None, 1)
