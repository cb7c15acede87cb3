"""Learned reranking without a GPU: the fifteenth header and its symbol table, every refusal of the two entry points (none reaches
a device), the limits that pass, ForestModel's checks, the feature resolver, every ValueError of the doors, a two-tree case worked
by hand, and scikit-learn models against the restatement (leaf for leaf, and within the fp32 bound of predict)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ltr_ref
import sparse_rx
from sparse_rx import _capi, ltr
from sparse_rx.backend import SparseBackend
from sparse_rx.fields import host_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(24)]  # 16-byte aligned addresses, never dereferenced

OTHER_TABLES = {"SYMBOLS": 35, "RESCORE_SYMBOLS": 4, "QUANT_SYMBOLS": 4, "FILTER_SYMBOLS": 8, "HALF_SYMBOLS": 5, "MMR_SYMBOLS": 3, "TERMS_SYMBOLS": 2,
                "MAXSIM_SYMBOLS": 3, "FIELDS_SYMBOLS": 1, "COLLAPSE_SYMBOLS": 1, "FACET_SYMBOLS": 2, "FEEDBACK_SYMBOLS": 2, "ORDER_SYMBOLS": 3,
                "BOOST_SYMBOLS": 1}


def test_fifteenth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "ltr", "sparse_rx_ltr.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef SPARSE_RX_LTR_H")[1]))
    assert declared == set(_capi.LTR_SYMBOLS) == {"srx_ltr_topk", "srx_ltr_score"}
    assert '#include "sparse_rx_fields.h"' in hdr
    assert len(OTHER_TABLES) == 14
    for name, size in OTHER_TABLES.items():
        table = getattr(_capi, name)
        assert len(table) == size, name
        assert not set(_capi.LTR_SYMBOLS) & set(table)
    assert sum(OTHER_TABLES.values()) + len(_capi.LTR_SYMBOLS) == 76
    assert os.listdir(os.path.join(ROOT, "include", "ltr")) == ["sparse_rx_ltr.h"]
    assert "ltr.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "ltr", "sparse_rx_ltr.h") in _capi._deps()
    assert "include/ltr/sparse_rx_ltr.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read().split('"""')[1]
    assert "include/ltr/sparse_rx_ltr.h" in _capi.__doc__
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.LTR_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert len(_capi.LTR_SYMBOLS["srx_ltr_topk"][1]) == len(inspect.signature(_topk).parameters) - 1 == 27
    assert len(_capi.LTR_SYMBOLS["srx_ltr_score"][1]) == len(inspect.signature(_score).parameters) - 1 == 23
    for name, value, ref in (("SRX_LTR_F_SCORE", 0, "F_SCORE"), ("SRX_LTR_F_RANK", 1, "F_RANK"), ("SRX_LTR_F_COLUMN", 2, "F_COLUMN"),
                             ("SRX_LTR_F_EXTRA", 3, "F_EXTRA"), ("SRX_LTR_LE", 0, "LE"), ("SRX_LTR_LT", 1, "LT"), ("SRX_LTR_REPLACE", 0, "REPLACE"),
                             ("SRX_LTR_SUM", 1, "SUM")):
        assert re.search(rf"\b{name} = {value}\b", hdr) and getattr(_capi, name) == value == getattr(ltr_ref, ref), name
    for name, value, ref in (("SRX_LTR_MISSING_LEFT", 1 << 30, "MISSING_LEFT"), ("SRX_LTR_MAX_M", 2048, "MAX_M"), ("SRX_LTR_MAX_COLS", 8, "MAX_COLS"),
                             ("SRX_LTR_MAX_FEATURES", 32, "MAX_FEATURES"), ("SRX_LTR_MAX_EXTRA", 32, "MAX_EXTRA"), ("SRX_LTR_MAX_TREES", 4096, "MAX_TREES"),
                             ("SRX_LTR_MAX_NODES", 1 << 22, "MAX_NODES")):
        assert re.search(rf"#define {name} {value}\b", hdr) and getattr(_capi, name) == value == getattr(ltr_ref, ref), name
    # the two structs: the same sizes and field order in the header, in ctypes, in the module's dtype and in the restatement's
    assert ctypes.sizeof(_capi.LtrNode) == 16 == ltr.NODE_DTYPE.itemsize == ltr_ref.NODE_DTYPE.itemsize == ltr_ref.NODE_BYTES
    assert ctypes.sizeof(_capi.LtrFeature) == 8 == ltr_ref.FEATURE_BYTES and "16 bytes" in hdr and "8 bytes" in hdr
    assert ltr.NODE_DTYPE == ltr_ref.NODE_DTYPE
    for name, _ in _capi.LtrNode._fields_:
        assert getattr(_capi.LtrNode, name).offset == ltr.NODE_DTYPE.fields[name][1], name
    assert [n for n, _ in _capi.LtrNode._fields_] == list(ltr.NODE_DTYPE.names) == re.findall(
        r"^\s+(?:int32_t|float) (\w+);", hdr.split("typedef struct srx_ltr_node")[1].split("}")[0], re.M)
    assert [n for n, _ in _capi.LtrFeature._fields_] == re.findall(r"^\s+int32_t (\w+);", hdr.split("typedef struct srx_ltr_feature")[1].split("}")[0], re.M)
    assert (ltr_ref.I32, ltr_ref.I64, ltr_ref.F32, ltr_ref.SET64) == (_capi.SRX_FIELD_I32, _capi.SRX_FIELD_I64, _capi.SRX_FIELD_F32, _capi.SRX_FIELD_SET64)
    assert ltr.CMPS == {"le": 0, "lt": 1} and ltr.MODES == {"replace": 0, "sum": 1}
    assert sparse_rx.ForestModel is ltr.ForestModel and {"ltr", "ForestModel", "RankFn"} <= set(sparse_rx.__all__)


# ---- every refusal of the calls -----------------------------------------------------------------------------------------------------
def _cols(*descs):
    arr = (_capi.FieldColDesc * max(len(descs), 1))()
    for i, (data, valid, typ) in enumerate(descs):
        arr[i].data, arr[i].valid, arr[i].type = data, valid, typ
    return arr


def _feats(*records):
    arr = (_capi.LtrFeature * max(len(records), 1))()
    for i, (kind, index) in enumerate(records):
        arr[i].kind, arr[i].index = kind, index
    return arr


DEFAULT_FEATS = ((0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (3, 2))


def _topk(L, device=0, cols=None, n_cols=2, n_docs=1000, doc_base=0, features=None, n_features=6, extra=P[3], n_extra=3, nodes=P[4], n_nodes=50,
          tree_ptr=P[5], n_trees=4, base=0.5, cmp=0, mode=0, cand_doc=P[6], cand_score=P[7], cand_count=P[8], nq=3, m=100, k=10, out_doc=P[12],
          out_score=P[13], out_count=P[14], out_pos=P[15], stream=None):
    if cols is None:
        cols = _cols((P[0], P[1], 1), (P[2], None, 2))
    if features is None:
        features = _feats(*DEFAULT_FEATS)
    return L.srx_ltr_topk(device, cols, n_cols, n_docs, doc_base, features, n_features, extra, n_extra, nodes, n_nodes, tree_ptr, n_trees, base, cmp, mode,
                          cand_doc, cand_score, cand_count, nq, m, k, out_doc, out_score, out_count, out_pos, stream)


def _score(L, device=0, cols=None, n_cols=2, n_docs=1000, doc_base=0, features=None, n_features=6, extra=P[3], n_extra=3, nodes=P[4], n_nodes=50,
           tree_ptr=P[5], n_trees=4, base=0.5, cmp=0, mode=0, cand_doc=P[6], cand_score=P[7], cand_count=P[8], nq=3, m=100, out_score=P[13], stream=None):
    if cols is None:
        cols = _cols((P[0], P[1], 1), (P[2], None, 2))
    if features is None:
        features = _feats(*DEFAULT_FEATS)
    return L.srx_ltr_score(device, cols, n_cols, n_docs, doc_base, features, n_features, extra, n_extra, nodes, n_nodes, tree_ptr, n_trees, base, cmp, mode,
                           cand_doc, cand_score, cand_count, nq, m, out_score, stream)


def refusals():
    """Every refusal of ``srx_ltr_topk`` and ``srx_ltr_score``: all return SRX_ERR_INVALID with their message, none touches a device
    (the pointers are never dereferenced); then the limits that pass, on nq == 0.  tests/test_ltr_gpu.py runs the same list on the
    GPU machine."""
    L = _capi.lib()
    null_cols = ctypes.cast(None, ctypes.POINTER(_capi.FieldColDesc))
    null_feats = ctypes.cast(None, ctypes.POINTER(_capi.LtrFeature))

    def refused(rc, word, who):
        msg = L.srx_last_error()
        assert rc == -1 and word.encode() in msg and msg.startswith(who.encode()), (rc, msg, word)

    for call, who in ((_topk, "srx_ltr_topk"), (_score, "srx_ltr_score")):
        no = lambda rc, word: refused(rc, word, who)
        no(call(L, cols=null_cols), "null cols")
        for n in (-1, 9, 33):
            no(call(L, n_cols=n), "n_cols must be in [0, 8]")
        no(call(L, cols=_cols((P[0], None, 3), (P[2], None, 2))), "SET64")
        no(call(L, cols=_cols((P[0], None, 0), (P[2], None, 3))), "SET64")
        for typ in (-1, 4, 99):
            no(call(L, cols=_cols((P[0], None, typ), (P[2], None, 2))), "unknown column type")
        for typ in (0, 1, 2):
            no(call(L, cols=_cols((None, None, typ), (P[2], None, 2))), "null data")
        for typ, off in ((0, 2), (0, 1), (2, 2), (1, 4), (1, 2)):
            no(call(L, cols=_cols((P[0], None, 0), (P[2] + off, None, typ))), "aligned for its type")
        for off in (4, 8, 2):
            no(call(L, cols=_cols((P[0], P[1] + off, 0), (P[2], None, 2))), "validity row must be 16-byte aligned")
        for n in (0, -3, 2 ** 31 - 1, 2 ** 40):
            no(call(L, n_docs=n), "n_docs must be in [1, 2^31 - 2]")
        no(call(L, doc_base=-1), "negative doc_base")
        no(call(L, features=null_feats), "null features")
        for n in (0, -1, 33):
            no(call(L, n_features=n), "n_features must be in [1, 32]")
        for n in (-1, 33):
            no(call(L, n_extra=n), "n_extra must be in [0, 32]")
        for kind in (-1, 4, 99):
            no(call(L, features=_feats((0, 0), (kind, 0)), n_features=2), "unknown feature kind")
        for index in (-1, 2, 8):
            no(call(L, features=_feats((2, index)), n_features=1), "COLUMN feature's index must be in [0, n_cols)")
        no(call(L, features=_feats((2, 0)), n_features=1, n_cols=0, cols=null_cols), "COLUMN feature's index must be in [0, n_cols)")
        for index in (-1, 3, 32):
            no(call(L, features=_feats((3, index)), n_features=1), "EXTRA feature's index must be in [0, n_extra)")
        no(call(L, features=_feats((3, 0)), n_features=1, n_extra=0), "EXTRA feature's index must be in [0, n_extra)")
        for n in (0, -1, 4097):
            no(call(L, n_trees=n), "n_trees must be in [1, 4096]")
        for n in (0, -1, (1 << 22) + 1):
            no(call(L, n_nodes=n), "n_nodes must be in [1, 2^22]")
        for c in (-1, 2, 99):
            no(call(L, cmp=c), "unknown cmp")
        for mode in (-1, 2, 99):
            no(call(L, mode=mode), "unknown mode")
        for m in (0, -1, 2049, 2 ** 31 - 1):
            no(call(L, m=m, **({"k": 1} if call is _topk else {})), "m must be in [1, 2048]")
        no(call(L, nq=-1), "nq < 0")
        no(call(L, nq=2 ** 31 - 1, m=2048), "nq * m must not exceed 2^31 - 1")
        for name in ("cand_doc", "cand_score"):
            no(call(L, **{name: None}), "null cand_doc / cand_score")
        for name in ("nodes", "tree_ptr"):
            no(call(L, **{name: None}), "null nodes / tree_ptr")
        for off in (4, 8, 12, 1):
            no(call(L, nodes=P[4] + off), "nodes must be 16-byte aligned")
        no(call(L, extra=None), "an EXTRA feature needs the extra plane")
        # what passes, on nq == 0 (no launch, whatever the device pointers are): the limits, no column, no extra, NULL count / pos
        nothing = dict(nq=0, cand_doc=None, cand_score=None, nodes=None, tree_ptr=None, extra=None, out_score=None)
        assert call(L, **nothing) == 0 and call(L, nq=0) == 0
        assert call(L, **nothing, n_cols=0, cols=null_cols, features=_feats((0, 0), (1, 0), (3, 31)), n_features=3, n_extra=32) == 0
        assert call(L, **nothing, n_cols=8, cols=_cols(*[(P[0], None, 0)] * 8), features=_feats(*[(2, 7)] * 32), n_features=32, n_extra=0) == 0
        assert call(L, **nothing, n_trees=4096, n_nodes=1 << 22, m=2048, n_docs=2 ** 31 - 2, doc_base=2 ** 40, cmp=1, mode=1) == 0
        assert call(L, **nothing, m=1, cand_count=None, **({"k": 1} if call is _topk else {})) == 0
    for k in (0, -1, 101):
        refused(_topk(L, k=k), "k must be in [1, m]", "srx_ltr_topk")
    for name in ("out_doc", "out_score", "out_count"):
        refused(_topk(L, **{name: None}), "null out_doc / out_score / out_count", "srx_ltr_topk")
    refused(_score(L, out_score=None), "null out_score", "srx_ltr_score")
    assert _topk(L, nq=0, k=100, out_pos=None, out_doc=None, out_count=None) == 0 and _topk(L, nq=0, m=2048, k=2048) == 0


def test_entry_point_refusals():
    refusals()


# ---- ForestModel ------------------------------------------------------------------------------------------------------------------
def two_trees(cmp="le"):
    """tree 0: x0 <= 1.5 ? (x2 <= 10 ? 1.0 : 2.0) : 4.0, a missing x0 goes left; tree 1: the root leaf 0.25"""
    return ltr.ForestModel.from_arrays(feature=[0, 2, -1, -1, -1, -1], value=[1.5, 10.0, 1.0, 2.0, 4.0, 0.25], left=[1, 2, 0, 0, 0, 0], right=[4, 3, 0, 0, 0, 0],
                                       tree_ptr=[0, 5, 6], base=0.125, cmp=cmp, default_left=[True, False, False, False, False, False])


def test_two_trees_by_hand():
    mdl = two_trees()
    assert (mdl.n_trees, mdl.n_nodes, mdl.n_features, float(mdl.base), mdl.cmp) == (2, 6, 3, 0.125, "le")
    assert mdl.nodes["feature"].tolist() == [(1 << 30) | 0, 2, -1, -1, -1, -1] and mdl.tree_ptr.tolist() == [0, 5, 6]
    score = lambda x, cmp=ltr_ref.LE, mode=ltr_ref.REPLACE, s=3.0: float(ltr_ref.model_score(mdl.nodes, mdl.tree_ptr, mdl.base, cmp, mode, 3, x, s))
    nan = float("nan")
    assert score([1.0, 0.0, 5.0]) == 0.125 + 1.0 + 0.25
    assert score([1.0, 0.0, 10.0]) == 0.125 + 1.0 + 0.25 and score([1.0, 0.0, 10.0], ltr_ref.LT) == 0.125 + 2.0 + 0.25  # x == threshold
    assert score([1.5, 0.0, 11.0]) == 0.125 + 2.0 + 0.25 and score([1.5, 0.0, 11.0], ltr_ref.LT) == 0.125 + 4.0 + 0.25
    assert score([2.0, 0.0, 0.0]) == 0.125 + 4.0 + 0.25
    assert score([nan, 0.0, nan]) == 0.125 + 2.0 + 0.25  # x0 missing: left (bit 30); x2 missing: right (no bit)
    assert score([1.0, 0.0, 5.0], mode=ltr_ref.SUM) == 3.0 + 1.375
    assert ltr_ref.leaves(mdl.nodes, mdl.tree_ptr, ltr_ref.LE, 3, [1.0, 0.0, 5.0]) == [2, 0]
    # fewer features than the model names: the tree that asks for one contributes +0
    assert float(ltr_ref.model_score(mdl.nodes, mdl.tree_ptr, mdl.base, ltr_ref.LE, ltr_ref.REPLACE, 2, [1.0, 0.0], 0.0)) == 0.125 + 0.0 + 0.25
    # the whole call: two queries, a dead doc, a count, ties by doc id, out_pos
    doc = np.array([[1007, 1003, 999, 1001], [1001, 1002, 1003, 1004]], np.int32)
    s = np.array([[1.0, 1.0, 1.0, 2.0], [9.0, 9.0, 9.0, 9.0]], np.float32)
    col = np.arange(10, dtype=np.int64) * 3  # doc 1003 -> 9, 1007 -> 21, 1001 -> 3
    feats = [(ltr_ref.F_SCORE, 0), (ltr_ref.F_RANK, 0), (ltr_ref.F_COLUMN, 0)]
    od, ob, oc, op = ltr_ref.ltr_topk([(ltr_ref.I64, col, None)], 10, 1000, feats, None, mdl.nodes, mdl.tree_ptr, mdl.base, ltr_ref.LE, ltr_ref.REPLACE,
                                      doc, s, np.array([4, 2], np.int32), 3)
    assert oc.tolist() == [3, 2] and od.tolist() == [[1001, 1007, 1003], [1001, 1002, -1]] and op.tolist() == [[3, 0, 1], [0, 1, -1]]
    assert ob.view(np.float32).tolist() == [[4.375, 2.375, 1.375], [4.375, 4.375, 0.0]]


def test_from_arrays_refusals():
    ok = dict(feature=[0, -1, -1], value=[0.5, 1.0, 2.0], left=[1, 0, 0], right=[2, 0, 0], tree_ptr=[0, 3])
    assert ltr.ForestModel.from_arrays(**ok).n_features == 1
    assert ltr.ForestModel.from_arrays([-1], [2.0], [0], [0], [0, 1]).n_features == 0  # a root leaf alone
    assert ltr.ForestModel.from_arrays(**{**ok, "value": [float("inf"), 1.0, 2.0]}).n_nodes == 3  # a threshold may be anything
    bad = [{"left": [0, 0, 0]}, {"left": [3, 0, 0]}, {"right": [-1, 0, 0]}, {"right": [2 ** 31, 0, 0]}, {"feature": [32, -1, -1]},
           {"feature": [70000, -1, -1]}, {"value": [0.5, float("nan"), 2.0]}, {"value": [0.5, 1.0, float("inf")]}, {"value": [0.5, 1.0, 1e39]},
           {"tree_ptr": [0, 2]}, {"tree_ptr": [1, 3]}, {"tree_ptr": [0, 3, 3]}, {"tree_ptr": [0, 0, 3]}, {"tree_ptr": [0]}, {"tree_ptr": [0, 2, 3], "left": [1, 0, 0]},
           {"base": float("nan")}, {"base": 1e39}, {"cmp": "ge"}, {"default_left": [True]}, {"value": [1, 2, 3]}, {"feature": [0.0, -1.0, -1.0]},
           {"left": [1, 0]}, {"tree_ptr": list(range(0, 4098))}]
    for change in bad:
        with pytest.raises(ValueError):
            ltr.ForestModel.from_arrays(**{**ok, **change})
    # a child inside ANOTHER tree is outside its own
    with pytest.raises(ValueError, match="strictly ahead"):
        ltr.ForestModel.from_arrays([0, -1, -1, -1], [0.5, 1, 2, 3], [1, 0, 0, 0], [3, 0, 0, 0], [0, 3, 4], base=0.0)


def _columns(n=30):
    return host_columns({"date": np.arange(n, dtype=np.int64), "votes": np.arange(n, dtype=np.int32), "price": np.arange(n, dtype=np.float32),
                         "tags": [["a"]] * n, **{f"c{i}": np.arange(n, dtype=np.int32) for i in range(8)}})


def test_resolve_features():
    cols = _columns()
    rec, names, n_extra = ltr.resolve_features(cols, ["score", "rank", "votes", ("extra", 4), "date", "votes", ("extra", 0)])
    assert rec == [(0, 0), (1, 0), (2, 0), (3, 4), (2, 1), (2, 0), (3, 0)] and names == ["votes", "date"] and n_extra == 5
    assert ltr.resolve_features(None, ["rank"]) == ([(1, 0)], [], 0)
    rec, names, n_extra = ltr.resolve_features(cols, ["dense_score", "sparse_score", ("extra", 1)], named_extra=ltr.HYBRID_FEATURES)
    assert rec == [(3, 1), (3, 0), (3, 3)] and n_extra == 4
    arr = ltr.feature_array(rec)
    assert [(a.kind, a.index) for a in arr] == rec
    for feats, word in ((None, "1 to 32"), ([], "1 to 32"), (["score"] * 33, "1 to 32"), ("score", "1 to 32"), (["nope"], "unknown field"), (["tags"], "set column"),
                        ([("extra", 32)], "outside"), ([("extra", -1)], "outside"), ([("extra", True)], "a feature is"), ([("column", 0)], "a feature is"),
                        ([3], "a feature is"), ([f"c{i}" for i in range(8)] + ["date"], "at most 8 columns"), (["sparse_score"], "search_hybrid"),
                        (["dense_score"], "search_hybrid")):
        with pytest.raises(ValueError, match=word):
            ltr.resolve_features(cols, feats)
    with pytest.raises(ValueError, match="needs doc fields"):
        ltr.resolve_features(None, ["date"])
    with pytest.raises(ValueError, match="the list has 2 features"):
        ltr.resolve_features(cols, ["score", "rank"], two_trees())
    with pytest.raises(ValueError, match="ForestModel"):
        ltr.resolve_features(cols, ["score"], object())
    # columns not known yet: any other name counts as a number column, the list's shape is still checked
    assert ltr.resolve_features(None, ["score", "later", "tags", "later"], any_column=True) == ([(0, 0), (2, 0), (2, 1), (2, 0)], ["later", "tags"], 0)
    with pytest.raises(ValueError, match="at most 8 columns"):
        ltr.resolve_features(None, [f"x{i}" for i in range(9)], any_column=True)
    with pytest.raises(ValueError, match="search_hybrid"):
        ltr.resolve_features(None, ["dense_score"], any_column=True)


# ---- the doors' refusals (no device is reached) -----------------------------------------------------------------------------------
def test_door_refusals():
    be = SparseBackend.__new__(SparseBackend)
    be._fields, be.host, be.dev, be.group, be._field_table, be._rank_model, be.n_docs_total = None, None, None, None, None, None, 30
    be.sharded = lambda: False
    mdl = two_trees()
    assert be.rank_spec(False) is None and be.rank_spec(None) is None and be.rank_spec(False, 10) is None
    with pytest.raises(ValueError, match="set_rank_model"):
        be.rank_spec(True, call="search_bm25")
    with pytest.raises(ValueError, match="ForestModel"):
        be.set_rank_model(object(), ["score"])
    with pytest.raises(ValueError, match="the list has 1 features"):
        be.set_rank_model(mdl, ["score"])
    with pytest.raises(ValueError, match="1 to 32"):
        be.set_rank_model(mdl, "score")
    be.set_rank_model(mdl, ["score", "rank", "date"])  # the fields may come later ...
    with pytest.raises(ValueError, match="set_doc_fields"):  # ... but a call that names a column needs them
        be.rank_spec(True, call="search_bm25")
    be._fields = _columns()
    fn = be.rank_spec(True, None, 10, "search_bm25")
    assert isinstance(fn, ltr.RankFn) and fn.pool == 30 and be.rank_spec(True, 7, 10).pool == 7 and fn.named_extra == ()
    with pytest.raises(ValueError, match="rank_pool"):
        be.rank_spec(True, 1025)
    with pytest.raises(ValueError, match="rank_pool"):
        be.rank_spec(True, 0)
    with pytest.raises(ValueError, match="boost="):
        be.rank_spec(True, None, 10, "search_bm25", boost=object())
    with pytest.raises(ValueError, match="set column"):
        be.set_rank_model(mdl, ["score", "rank", "tags"])
    with pytest.raises(ValueError, match="unknown field"):
        be.set_rank_model(mdl, ["score", "rank", "nope"])
    be._rank_model = (mdl, ["score", "rank", "tags"])  # set before the fields were: the call refuses
    with pytest.raises(ValueError, match="set column"):
        be.rank_spec(True)
    be.set_rank_model(mdl, ["sparse_score", "dense_score", "date"])
    with pytest.raises(ValueError, match="search_hybrid"):
        be.rank_spec(True, call="search_bm25")
    with pytest.raises(ValueError, match="search_hybrid"):
        be.rerank_model_results({"q": {}}, 3)
    assert be.rank_spec(True, call="search_hybrid", hybrid=True).named_extra == ltr.HYBRID_FEATURES
    be.set_rank_model(mdl, ["sparse_score", "dense_score", ("extra", 0)])  # a hybrid search has no further extras to give
    with pytest.raises(ValueError, match="cannot fill"):
        be.rank_spec(True, call="search_hybrid", hybrid=True)
    be.set_rank_model(mdl, ["score", "rank", ("extra", 0)])
    with pytest.raises(ValueError, match="cannot fill"):
        be.rank_spec(True, call="search_hybrid", hybrid=True)
    assert be.rank_spec(True, call="search_bm25").named_extra == ()
    be.set_rank_model(mdl, ["score", "rank", "date"])
    assert be.rank_spec(True, call="search_hybrid", hybrid=True).named_extra == ()
    with pytest.raises(ValueError, match="mode must be"):
        be.rerank_model_results({"q": {}}, 3, mode="multiply")
    with pytest.raises(ValueError, match="top_k must be >= 1"):
        be.rerank_model_results({"q": {}}, 0)
    assert be.rerank_model_results({}, 3) == {}
    be.sharded = lambda: True
    with pytest.raises(ValueError, match="one GPU"):
        be.rank_spec(True)
    # the keywords exist on the doors the issue names, last, with defaults that change nothing, and not on the others
    for fn in (sparse_rx.RetrievalService.search_bm25, sparse_rx.OptimizedBM25Retriever.search, sparse_rx.OptimizedRetriever.search,
               sparse_rx.RetrievalService.search_hybrid):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["rank_model", "rank_pool"] and p["rank_model"].default is False and p["rank_pool"].default is None
    for cls in (sparse_rx.RetrievalService, sparse_rx.OptimizedBM25Retriever, sparse_rx.OptimizedRetriever):
        assert list(inspect.signature(cls.rerank_model).parameters) == ["self", "results", "top_k", "extra", "mode"]
        assert list(inspect.signature(cls.set_rank_model).parameters) == ["self", "model", "features"]
    for fn in (sparse_rx.HybridRetriever.search, sparse_rx.ShardedSearcher.search, sparse_rx.HostBatchPipeline.search):
        assert "rank_model" not in inspect.signature(fn).parameters


def test_mirrors_take_the_old_path_without_the_keywords():
    """rank_model=False hands the call to search_dicts exactly as before: the same arguments, no model looked at"""
    seen = []

    class Be:
        n_docs_total = 5
        filter_spec = collapse_spec = expand_spec = boost_spec = staticmethod(lambda *a, **k: None)

        def rank_spec(self, rank_model, rank_pool=None, top_k=10, call="search", boost=None, hybrid=False):
            assert not rank_model
            return SparseBackend.rank_spec(self, rank_model, rank_pool, top_k, call, boost, hybrid)

        def search_dicts(self, queries, top_k, **kw):
            seen.append((queries, top_k, kw))
            return {"q": {"d": 1.0}}

    for cls, name in ((sparse_rx.RetrievalService, "search_bm25"), (sparse_rx.OptimizedBM25Retriever, "search"), (sparse_rx.OptimizedRetriever, "search")):
        obj = cls.__new__(cls)
        obj._be, obj.query_cache, obj.cache_lock, obj.k1, obj.b, obj._built_k1b = Be(), {}, None, 1.2, 0.75, (1.2, 0.75)
        obj._need_index = lambda: None
        if cls is sparse_rx.OptimizedRetriever:
            obj.term_order = "token"
        assert getattr(obj, name)({"q": "text"}, 3) == {"q": {"d": 1.0}}
        queries, top_k, kw = seen.pop()
        assert queries == {"q": "text"} and top_k == 3 and kw["filter"] is None and kw["collapse"] is None and kw["expand"] is None and kw["boost"] is None
        assert "rank_model" not in kw and "rank" not in kw


# ---- scikit-learn ---------------------------------------------------------------------------------------------------------------
def _sk_data(n=4000, seed=0):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.standard_normal(n) * 3, rng.integers(0, 50, n).astype(np.float64), rng.random(n) * 1000, rng.standard_normal(n),
                  rng.integers(-5, 5, n).astype(np.float64), rng.random(n)], axis=1).astype(np.float32)
    y = np.where(X[:, 0] > 0.5, 2.0, -1.0) + 0.05 * X[:, 1] + np.sin(X[:, 2] / 100.0) + 0.3 * X[:, 3] * (X[:, 4] > 0) + rng.standard_normal(n) * 0.1
    return X, y


def _on_thresholds(est, X):
    """Rows placed exactly on float32-rounded thresholds of the model's splits: the compare's edge"""
    trees = [t for row in np.atleast_2d(np.asarray(est.estimators_, dtype=object)) for t in np.atleast_1d(row)] if hasattr(est, "estimators_") else [est]
    rows = []
    for t in trees[:10]:
        tr = t.tree_
        for i in np.flatnonzero(tr.children_left >= 0)[:6]:
            for v in (np.float32(tr.threshold[i]), np.nextafter(np.float32(tr.threshold[i]), np.float32(np.inf)),
                      np.nextafter(np.float32(tr.threshold[i]), np.float32(-np.inf))):
                row = X[len(rows) % len(X)].copy()
                row[tr.feature[i]] = v
                rows.append(row)
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("kind", ["gbr", "rf", "tree"])
def test_from_sklearn_walks_like_sklearn(kind):
    pytest.importorskip("sklearn")
    from sklearn.ensemble import GradientBoostingRegressor, RandomForestRegressor
    from sklearn.tree import DecisionTreeRegressor
    X, y = _sk_data()
    est = {"gbr": GradientBoostingRegressor(n_estimators=40, max_depth=4, learning_rate=0.1, random_state=0),
           "rf": RandomForestRegressor(n_estimators=30, max_depth=6, random_state=0, n_jobs=1), "tree": DecisionTreeRegressor(max_depth=7, random_state=0)}[kind].fit(X, y)
    mdl = ltr.ForestModel.from_sklearn(est)
    T = mdl.n_trees
    assert T == {"gbr": 40, "rf": 30, "tree": 1}[kind] and mdl.cmp == "le" and mdl.n_features <= 6
    assert float(mdl.base) == (float(np.float32(est.init_.constant_[0, 0])) if kind == "gbr" else 0.0)
    rows = np.concatenate([X, _on_thresholds(est, X)])
    applied = est.apply(rows)  # gbr: [n, T, 1]; rf: [n, T]; tree: [n]
    applied = np.asarray(applied).reshape(len(rows), T)
    want = est.predict(rows)
    mismatches, worst = 0, np.inf
    for r in range(len(rows)):
        x = rows[r]
        got_leaves = ltr_ref.leaves(mdl.nodes, mdl.tree_ptr, ltr_ref.LE, 6, x)
        mismatches += int(got_leaves != applied[r].tolist())
        got = float(ltr_ref.model_score(mdl.nodes, mdl.tree_ptr, mdl.base, ltr_ref.LE, ltr_ref.REPLACE, 6, x, 0.0))
        mass = abs(float(mdl.base)) + sum(abs(float(mdl.nodes["value"][int(mdl.tree_ptr[t]) + l])) for t, l in enumerate(got_leaves))
        bound = (T + 2) * 2.0 ** -24 * mass
        assert abs(got - float(want[r])) <= bound, (r, got, float(want[r]), bound)
        worst = min(worst, bound - abs(got - float(want[r])))
    assert mismatches == 0 and worst > 0.0


def test_from_sklearn_missing_values_and_refusals():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import ExtraTreesRegressor, GradientBoostingClassifier, RandomForestRegressor
    from sklearn.linear_model import LinearRegression
    from sklearn.tree import DecisionTreeClassifier, DecisionTreeRegressor
    X, y = _sk_data(600, seed=1)
    Xm = X.copy()
    Xm[::7, 0] = np.nan
    Xm[::5, 2] = np.nan
    est = DecisionTreeRegressor(max_depth=6, random_state=0).fit(Xm, y)
    mdl = ltr.ForestModel.from_sklearn(est)
    assert (mdl.nodes["feature"][mdl.nodes["feature"] >= 0] & (1 << 30)).any() or not est.tree_.missing_go_to_left.any()
    applied = est.apply(Xm)
    for r in range(len(Xm)):
        assert ltr_ref.leaves(mdl.nodes, mdl.tree_ptr, ltr_ref.LE, 6, Xm[r]) == [int(applied[r])]
    for bad in (DecisionTreeClassifier(max_depth=2).fit(X, (y > 0).astype(int)), GradientBoostingClassifier(n_estimators=2).fit(X, (y > 0).astype(int)),
                RandomForestRegressor(n_estimators=2, max_depth=2).fit(X, np.stack([y, y], axis=1)), LinearRegression().fit(X, y), ExtraTreesRegressor(n_estimators=2, max_depth=2).fit(X, y), object()):
        with pytest.raises(ValueError):
            ltr.ForestModel.from_sklearn(bad)
