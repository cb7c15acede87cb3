"""Learned reranking (include/ltr/sparse_rx_ltr.h): a tree-ensemble model -- LambdaMART, gradient boosting, a random forest --
over the features the device already holds, applied to ranked lists by ``srx_ltr_topk`` / ``srx_ltr_score``.

:class:`ForestModel` is the node table of the header on the host, validated for what the device does not check (it walks ANY
table safely, but a malformed tree contributes +0 instead of failing); :meth:`ForestModel.from_sklearn` converts scikit-learn's
regressors so that the fp32 walk takes scikit-learn's own path for float32 inputs.  :func:`resolve_features` turns the feature names
of a door -- "score", "rank", a column of the field table, ``("extra", i)`` -- into the header's records; :class:`RankFn` is a model
bound to a :class:`~.fields.FieldTable`, its arrays uploaded once.

Loaders for other libraries are a mapping onto :meth:`ForestModel.from_arrays`: XGBoost splits on ``x < value``
(``cmp="lt"``) and numbers its nodes breadth-first, children after parents; LightGBM splits on ``x <= value`` (``cmp="le"``) and keeps
internal nodes and leaves in two arrays, which renumber into one with every child behind its parent."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _capi

NODE_DTYPE = np.dtype([("feature", "<i4"), ("value", "<f4"), ("left", "<i4"), ("right", "<i4")])  # srx_ltr_node, 16 bytes
FEATURE_KINDS = {"score": _capi.SRX_LTR_F_SCORE, "rank": _capi.SRX_LTR_F_RANK, "column": _capi.SRX_LTR_F_COLUMN, "extra": _capi.SRX_LTR_F_EXTRA}
CMPS = {"le": _capi.SRX_LTR_LE, "lt": _capi.SRX_LTR_LT}
MODES = {"replace": _capi.SRX_LTR_REPLACE, "sum": _capi.SRX_LTR_SUM}
HYBRID_FEATURES = ("sparse_score", "dense_score")  # names only search_hybrid fills (exact scores of the pool's docs)


def check_mode(mode) -> int:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    return MODES[mode]


class ForestModel:
    """A tree ensemble as ``srx_ltr_topk`` reads it: ``nodes`` (:data:`NODE_DTYPE` records), ``tree_ptr`` int32 [n_trees + 1],
    ``base`` float32, ``cmp`` "le" | "lt".  ``n_features``: one more than the largest feature index a split names (0: leaves only).
    Build one with :meth:`from_arrays` or :meth:`from_sklearn`; the constructor checks nothing."""

    def __init__(self, nodes: np.ndarray, tree_ptr: np.ndarray, base, cmp: str):
        self.nodes, self.tree_ptr, self.base, self.cmp = nodes, tree_ptr, np.float32(base), cmp
        split = nodes["feature"] >= 0
        self.n_features = int((nodes["feature"][split] & 0xFFFF).max()) + 1 if split.any() else 0
        self._device = {}

    n_trees = property(lambda self: len(self.tree_ptr) - 1)
    n_nodes = property(lambda self: len(self.nodes))

    @classmethod
    def from_arrays(cls, feature, value, left, right, tree_ptr, base=0.0, cmp: str = "le", default_left=None) -> "ForestModel":
        """Node ``i`` of the concatenated trees: ``feature[i]`` < 0 marks a leaf whose output is ``value[i]``; otherwise it is the
        index of the feature compared with the threshold ``value[i]`` (``cmp`` "le": x <= value goes left, "lt": x < value), and
        ``left[i]`` / ``right[i]`` are the children, numbered from the tree's first node.  ``tree_ptr`` [n_trees + 1]: tree t is the
        nodes ``tree_ptr[t] .. tree_ptr[t + 1]``.  ``default_left`` (bool per node, None: all False): a missing value (NaN) goes
        left.  Leaf values hold the learning rate, or 1 / n_trees of a forest, already: the device only adds.  ValueError for
        what the device does not refuse: a child not strictly ahead of its node or outside its tree, a feature index outside
        [0, 32), a leaf that is not finite, an empty tree, a ``tree_ptr`` that does not tile the nodes, more than 4 096 trees or
        2^22 nodes, a ``base`` that is not finite."""
        if cmp not in CMPS:
            raise ValueError(f"cmp must be \"le\" or \"lt\", got {cmp!r}")
        feature, left, right = (np.asarray(a) for a in (feature, left, right))
        value = np.asarray(value)
        for a, what in ((feature, "feature"), (left, "left"), (right, "right"), (np.asarray(tree_ptr), "tree_ptr")):
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError(f"{what} must be a 1-D integer array")
        n = len(feature)
        if value.ndim != 1 or value.dtype.kind != "f" or not (len(value) == len(left) == len(right) == n):
            raise ValueError("feature, value (floats), left and right must be 1-D arrays of one length")
        if not (1 <= n <= _capi.SRX_LTR_MAX_NODES):
            raise ValueError(f"a model takes 1 to 2^22 nodes, got {n}")
        tp = np.asarray(tree_ptr, dtype=np.int64)
        if not (2 <= len(tp) <= _capi.SRX_LTR_MAX_TREES + 1):
            raise ValueError(f"a model takes 1 to {_capi.SRX_LTR_MAX_TREES} trees, got {len(tp) - 1}")
        if tp[0] != 0 or tp[-1] != n or (np.diff(tp) < 1).any():
            raise ValueError("tree_ptr must start at 0, end at the node count and give every tree at least one node")
        with np.errstate(over="ignore"):
            base32 = np.float32(base)
        if not np.isfinite(base32):
            raise ValueError(f"base must be a finite float32, got {base!r}")
        feature = feature.astype(np.int64)
        leaf = feature < 0
        if (feature[~leaf] >= _capi.SRX_LTR_MAX_FEATURES).any():
            raise ValueError(f"a feature index must be in [0, {_capi.SRX_LTR_MAX_FEATURES})")
        with np.errstate(over="ignore"):
            v32 = value.astype(np.float32)
        if not np.isfinite(v32[leaf]).all():
            raise ValueError("every leaf value must be a finite float32")
        tree = np.searchsorted(tp, np.arange(n), side="right") - 1
        first, end = tp[tree], tp[tree + 1]
        here = np.arange(n)
        for child, what in ((left.astype(np.int64), "left"), (right.astype(np.int64), "right")):
            j = first + child
            bad = ~leaf & ~((j > here) & (j < end))
            if bad.any():
                i = int(np.flatnonzero(bad)[0])
                raise ValueError(f"node {i}: its {what} child {int(child[i])} is not strictly ahead of it inside its tree")
        nodes = np.zeros(n, dtype=NODE_DTYPE)
        dl = np.zeros(n, dtype=bool) if default_left is None else np.asarray(default_left).astype(bool)
        if dl.shape != (n,):
            raise ValueError("default_left must have one entry per node")
        nodes["feature"] = np.where(leaf, -1, feature | np.where(dl, _capi.SRX_LTR_MISSING_LEFT, 0)).astype(np.int32)
        nodes["value"] = v32
        nodes["left"], nodes["right"] = np.where(leaf, 0, left).astype(np.int32), np.where(leaf, 0, right).astype(np.int32)
        return cls(nodes, tp.astype(np.int32), base32, cmp)

    @classmethod
    def from_sklearn(cls, est) -> "ForestModel":
        """A fitted ``GradientBoostingRegressor``, ``RandomForestRegressor`` or ``DecisionTreeRegressor``.  ``cmp`` is "le", as
        scikit-learn's; a float64 threshold becomes the largest float32 not above it, so the fp32 compare decides as
        scikit-learn's compare of a float32 input with the float64 threshold does (:func:`~.fields.f32_at_most`); a leaf is
        ``float32(value * learning_rate)`` (a forest: ``value / n_estimators``), ``base`` the init constant, ``missing_go_to_left``
        bit 30.  ValueError: a classifier, a multi-output model, another estimator, an ``init`` estimator that is no constant."""
        from .fields import f32_at_most
        name = type(est).__name__
        if hasattr(est, "classes_") or name.endswith("Classifier"):
            raise ValueError(f"{name} is a classifier: a rank model is a single-output regressor")
        if int(getattr(est, "n_outputs_", 1)) != 1:
            raise ValueError(f"{name} has {est.n_outputs_} outputs: a rank model has one")
        if name == "GradientBoostingRegressor":
            trees, scale = [t for row in est.estimators_ for t in row], float(est.learning_rate)
            init = est.init_
            if isinstance(init, str):  # "zero"
                base = 0.0
            elif hasattr(init, "constant_"):
                base = float(np.asarray(init.constant_).ravel()[0])
            else:
                raise ValueError("GradientBoostingRegressor with an init estimator that is no constant")
        elif name == "RandomForestRegressor":
            trees, scale, base = list(est.estimators_), 1.0 / len(est.estimators_), 0.0
        elif name == "DecisionTreeRegressor":
            trees, scale, base = [est], 1.0, 0.0
        else:
            raise ValueError(f"from_sklearn takes a GradientBoostingRegressor, RandomForestRegressor or DecisionTreeRegressor, got {name}")
        feature, value, left, right, dleft, ptr = [], [], [], [], [], [0]
        for t in trees:
            tr = t.tree_
            leaf = tr.children_left < 0
            out = tr.value.reshape(tr.node_count, -1)[:, 0]
            if name == "RandomForestRegressor":
                leaves = out / float(len(trees))
            else:
                leaves = out * scale
            thr = np.asarray([0.0 if l else float(f32_at_most(float(x))) for l, x in zip(leaf, tr.threshold)], dtype=np.float32)
            feature.append(np.where(leaf, -1, tr.feature))
            value.append(np.where(leaf, leaves.astype(np.float32), thr))
            left.append(np.where(leaf, 0, tr.children_left))
            right.append(np.where(leaf, 0, tr.children_right))
            mg = getattr(tr, "missing_go_to_left", None)
            dleft.append(np.zeros(tr.node_count, bool) if mg is None else np.asarray(mg).astype(bool) & ~leaf)
            ptr.append(ptr[-1] + tr.node_count)
        return cls.from_arrays(np.concatenate(feature), np.concatenate(value).astype(np.float32), np.concatenate(left), np.concatenate(right), ptr,
                               base=np.float32(base), cmp="le", default_left=np.concatenate(dleft))

    def to_device(self, device):
        """``(nodes uint8 [n_nodes, 16], tree_ptr int32 [n_trees + 1])`` on ``device``, uploaded once per device"""
        import torch
        dev = torch.device(device)
        if dev not in self._device:
            self._device[dev] = (torch.as_tensor(self.nodes.view(np.uint8).reshape(-1, NODE_DTYPE.itemsize).copy(), device=dev),
                                 torch.as_tensor(self.tree_ptr.copy(), device=dev))
        return self._device[dev]


def resolve_features(columns, features, model: Optional[ForestModel] = None, named_extra: Sequence[str] = (), any_column: bool = False):
    """The ``features`` of a door -- a list of "score", "rank", the name of a number column of ``columns`` (name -> HostColumn; may
    be None or empty when no column is named), or ``("extra", i)`` -- as ``(records [(kind, index)], column names, n_extra)``: the
    columns in the order of their first use, n_extra one more than the largest extra index.  ``named_extra``: names that stand for
    the extra slots 0, 1, .. of a caller that fills them itself (search_hybrid's "sparse_score" / "dense_score"); a plain
    ``("extra", i)`` then counts from behind them.  ValueError: no or more than 32 features, an unknown name (one of
    :data:`HYBRID_FEATURES` outside ``named_extra``: it exists in search_hybrid only), a set column, more than 8 columns, an extra
    index outside [0, 32), a ``model`` that names a feature the list does not have.  ``any_column``: the columns are not known yet, so
    every other name counts as a number column (the list's shape is checked; the call that ranks resolves the names again)."""
    if model is not None and not isinstance(model, ForestModel):
        raise ValueError("model must be a ForestModel (ForestModel.from_arrays / from_sklearn)")
    feats = list(features) if isinstance(features, (list, tuple)) else None
    if not feats or len(feats) > _capi.SRX_LTR_MAX_FEATURES:
        raise ValueError(f"features must be a list of 1 to {_capi.SRX_LTR_MAX_FEATURES} names")
    named = list(named_extra)
    records: List[Tuple[int, int]] = []
    names: List[str] = []
    n_extra = len(named)
    for f in feats:
        if isinstance(f, (tuple, list)):
            if len(f) != 2 or f[0] != "extra" or isinstance(f[1], bool) or not isinstance(f[1], (int, np.integer)):
                raise ValueError(f"a feature is \"score\", \"rank\", a column name or (\"extra\", i), got {f!r}")
            i = int(f[1]) + len(named)
            if not (len(named) <= i < _capi.SRX_LTR_MAX_EXTRA):
                raise ValueError(f"extra index {int(f[1])} outside [0, {_capi.SRX_LTR_MAX_EXTRA - len(named)})")
            records.append((_capi.SRX_LTR_F_EXTRA, i))
            n_extra = max(n_extra, i + 1)
        elif not isinstance(f, str):
            raise ValueError(f"a feature is \"score\", \"rank\", a column name or (\"extra\", i), got {f!r}")
        elif f in named:
            records.append((_capi.SRX_LTR_F_EXTRA, named.index(f)))
        elif f in HYBRID_FEATURES:
            raise ValueError(f"the feature {f!r} exists in search_hybrid(rank_model=True) only: there the sparse and the dense score are both known")
        elif f == "score":
            records.append((_capi.SRX_LTR_F_SCORE, 0))
        elif f == "rank":
            records.append((_capi.SRX_LTR_F_RANK, 0))
        else:
            if not any_column and (not columns or f not in columns):
                raise ValueError(f"unknown field {f!r}" if columns else f"the feature {f!r} names a column: it needs doc fields")
            if not any_column and columns[f].kind == "set":
                raise ValueError(f"{f!r} is a set column: a label set is no number to rank by")
            if f not in names:
                names.append(f)
            records.append((_capi.SRX_LTR_F_COLUMN, names.index(f)))
    if len(names) > _capi.SRX_LTR_MAX_COLS:
        raise ValueError(f"a rank model takes at most {_capi.SRX_LTR_MAX_COLS} columns, got {len(names)}")
    if model is not None and model.n_features > len(records):
        raise ValueError(f"the model splits on feature {model.n_features - 1}, the list has {len(records)} features")
    return records, names, n_extra


def feature_array(records):
    """The HOST ``srx_ltr_feature`` array of :func:`resolve_features`' records"""
    arr = (_capi.LtrFeature * len(records))()
    for i, (kind, index) in enumerate(records):
        arr[i].kind, arr[i].index = int(kind), int(index)
    return arr


class RankFn:
    """A :class:`ForestModel` and its feature list bound to a :class:`~.fields.FieldTable`: ``fn(doc, score, count, k, extra=None, mode="replace", want_pos=False)`` ->
    ``(doc [nq, k], score [nq, k], count [nq])`` with the contract of ``srx_ltr_topk``.  The model goes to the device once."""

    def __init__(self, table, model: ForestModel, features, named_extra: Sequence[str] = (), columns=None):
        """``table``: the FieldTable, or a function without arguments that makes it at the first call (``columns``: its host columns
        then, so that the names are checked before a device is touched)"""
        self._table, self.model, self.features, self.named_extra = table, model, list(features) if isinstance(features, (list, tuple)) else features, tuple(named_extra)
        resolve_features(table.columns if columns is None else columns, self.features, model, self.named_extra)

    @property
    def table(self):
        if callable(self._table):
            self._table = self._table()
        return self._table

    def __call__(self, doc, score, count, k, extra=None, mode: str = "replace", want_pos: bool = False):
        return self.table.rank_model_device(self.model, self.features, doc, score, count, k, extra=extra, mode=mode, want_pos=want_pos,
                                            named_extra=self.named_extra)
