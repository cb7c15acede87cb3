"""Field-value boosts (include/boost/sparse_rx_boost.h): a boost spec resolved to the clause records and knot tables the device
reads, and the paged search that makes a boosted top k exact.

The device knows ONE function shape: a clamped, uniformly spaced, piecewise-linear curve over a signed or absolute offset from an
origin.  :class:`BoostResolver` samples what a caller asks for -- Elasticsearch's gauss / exp / linear decays, a
``field_value_factor`` with a modifier, or the caller's own table -- into such curves, in float64, and reports how far each table
lies from its formula (``max_dev``).  The table, not the formula, is the contract: tests/boost_ref.py restates what the device
computes from it bit for bit.  The reference has no score boosting: nothing here mirrors reference code.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np

from . import _capi
from .index import deep_reduce

SCORE_MODES = {"multiply": _capi.SRX_BOOST_SCORE_MULTIPLY, "sum": _capi.SRX_BOOST_SCORE_SUM, "max": _capi.SRX_BOOST_SCORE_MAX,
               "min": _capi.SRX_BOOST_SCORE_MIN}
BOOST_MODES = {"multiply": _capi.SRX_BOOST_MULTIPLY, "sum": _capi.SRX_BOOST_SUM, "replace": _capi.SRX_BOOST_REPLACE}
DECAY_KINDS = ("gauss", "exp", "linear")
MODIFIERS = {"none": lambda z: z, "log1p": np.log1p, "sqrt": np.sqrt, "square": lambda z: z * z}
FUNCTION_KINDS = ("decay", "field_value", "curve")
# the 40 bytes of srx_boost_clause
CLAUSE_DTYPE = np.dtype([("col", "<i4"), ("flags", "<i4"), ("origin", "<i8"), ("inv_step", "<f4"), ("weight", "<f4"), ("missing", "<f4"),
                         ("knot0", "<i4"), ("n_seg", "<i4"), ("reserved", "<i4")])
_DECAY_KEYS = {"field", "origin", "scale", "offset", "decay", "kind", "tail", "segments", "weight", "missing"}
_VALUE_KEYS = {"field", "lo", "hi", "modifier", "factor", "segments", "weight", "missing"}
_CURVE_KEYS = {"field", "origin", "step", "knots", "abs", "weight", "missing"}


def _finite(x, what: str) -> float:
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} must be a number, got {x!r}")
    x = float(x)
    if not math.isfinite(x):
        raise ValueError(f"{what} must be finite, got {x!r}")
    return x


def _f32(x, what: str) -> np.float32:
    with np.errstate(over="ignore"):
        f = np.float32(_finite(x, what))
    if not np.isfinite(f):
        raise ValueError(f"{what} = {x!r} is no finite float32")
    return f


def _segments(x, what: str) -> int:
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not (1 <= int(x) < _capi.SRX_BOOST_MAX_KNOTS):
        raise ValueError(f"{what} must be an integer in [1, 2^24), got {x!r}")
    return int(x)


def decay_value(kind: str, d, scale: float, decay: float):
    """Elasticsearch's decay functions of the distance ``d`` >= 0 beyond the offset (float64): ``decay`` at ``d == scale``"""
    d = np.asarray(d, dtype=np.float64)
    if kind == "gauss":
        return np.exp(d * d * (math.log(decay) / (scale * scale)))  # exp(-d^2 / (2 sigma^2)), sigma^2 = -scale^2 / (2 ln decay)
    if kind == "exp":
        return np.exp(d * (math.log(decay) / scale))
    return np.maximum(0.0, (scale / (1.0 - decay) - d) / (scale / (1.0 - decay)))


def decay_reach(kind: str, scale: float, decay: float, tail: float) -> float:
    """The distance beyond the offset at which the decay has fallen to ``tail`` (linear: to 0)"""
    if kind == "gauss":
        return scale * math.sqrt(math.log(tail) / math.log(decay))
    if kind == "exp":
        return scale * math.log(tail) / math.log(decay)
    return scale / (1.0 - decay)


class BoostFunction:
    """One resolved function: ``field``, ``abs``, ``origin`` (an int; a float32 column: the float's bits), ``inv_step`` (float32),
    ``knots`` (float32[n_seg + 1]), ``weight``, ``missing`` (float32) and ``max_dev`` (float64, None for a caller's table)."""

    def __init__(self, field, abs_, origin, inv_step, knots, weight, missing, max_dev):
        self.field, self.abs, self.origin, self.inv_step, self.knots = field, bool(abs_), int(origin), inv_step, knots
        self.weight, self.missing, self.max_dev = weight, missing, max_dev


def _sample(fn, inv_step: np.float32, n_seg: int, what: str):
    """The knots of ``fn`` (float64 -> float64 over the offset x >= 0) at x_j = j / inv_step -- the places the device's
    t = x * inv_step calls j -- as float32, and the largest |table - fn| at the segment midpoints, in float64."""
    step = 1.0 / float(inv_step)
    with np.errstate(all="ignore"):
        y64 = np.asarray(fn(np.arange(n_seg + 1, dtype=np.float64) * step), dtype=np.float64)
        knots = y64.astype(np.float32)
        if not np.isfinite(knots).all():
            raise ValueError(f"{what}: the curve is not finite over its range (a knot is {knots[~np.isfinite(knots)][0]!r})")
        mid = np.asarray(fn((np.arange(n_seg, dtype=np.float64) + 0.5) * step), dtype=np.float64)
    k64 = knots.astype(np.float64)
    return knots, float(np.max(np.abs(0.5 * (k64[:-1] + k64[1:]) - mid)))


def _origin_for(col, origin, what: str):
    """``origin`` as the clause holds it for ``col``: (the int64 field, the value it stands for as a float)"""
    if col.type == _capi.SRX_FIELD_F32:
        f = _f32(origin, what)
        return int(np.asarray(f, dtype=np.float32).view(np.uint32)), float(f)
    if isinstance(origin, (float, np.floating)):
        if not math.isfinite(float(origin)) or float(origin) != math.floor(float(origin)):
            raise ValueError(f"{what} = {origin!r}: an integer column takes an integral origin")
        origin = int(origin)
    if isinstance(origin, (bool, np.bool_)) or not isinstance(origin, (int, np.integer)) or not (-(2 ** 63) <= int(origin) < 2 ** 63):
        raise ValueError(f"{what} must be an integer inside int64, got {origin!r}")
    return int(origin), float(int(origin))


def _inv_step(step: float, what: str) -> np.float32:
    with np.errstate(all="ignore"):
        inv = np.float32(1.0 / step) if step > 0 and math.isfinite(step) else np.float32(np.nan)
    if not np.isfinite(inv) or not inv > 0:
        raise ValueError(f"{what}: the knot spacing {step!r} has no finite positive float32 inverse")
    return inv


class BoostResolver:
    """A boost spec ``{"functions": [...], "score_mode": "multiply", "boost_mode": "multiply"}`` resolved against ``columns`` (name ->
    :class:`~.fields.HostColumn`).  1 to 8 functions, each a dict with ONE key:

      * ``{"decay": {"field", "origin", "scale", "offset": 0, "decay": 0.5, "kind": "gauss" | "exp" | "linear", "tail": 1e-3,
        "segments": 256, "weight": 1, "missing": 1}}`` -- Elasticsearch's decay of ``max(0, |value - origin| - offset)``: ``decay``
        at the distance ``scale``.  Sampled out to where the curve reaches ``tail`` (linear: 0) and flat beyond.
      * ``{"field_value": {"field", "lo", "hi", "modifier": "none" | "log1p" | "sqrt" | "square", "factor": 1, "segments": 256
        (1 for "none"), "weight": 1, "missing": 1}}`` -- ``modifier(factor * value)`` with the value clamped to [lo, hi].
      * ``{"curve": {"field", "origin", "step", "knots", "abs": False, "weight": 1, "missing": 1}}`` -- the caller's table:
        knot j stands at the offset ``j * step`` from ``origin``.

    A doc without a value takes ``missing`` as the function's value (then times ``weight``).  ``score_mode`` folds the functions
    ("multiply", "sum", "max", "min"), ``boost_mode`` joins the fold F with the raw score ("multiply", "sum", "replace").

    Attributes: ``functions`` (:class:`BoostFunction`), ``names`` (the distinct columns, at most 8: what a clause's ``col`` indexes),
    ``clauses`` (the 40-byte records), ``knots`` (float32, all tables), ``score_mode`` / ``boost_mode`` (SRX_BOOST_*),
    ``max_dev`` (per function) and ``F_lo`` / ``F_hi``: float32 bounds of every F the device can compute, from the same fp32
    operations on per-clause extremes -- rounding is monotone.  A clause's extremes run over its knots, ``missing`` and, per
    segment, ``fl(y_i + fl(y_(i+1) - y_i))``: a rounded lerp stays between y_i and that value, which can lie one rounding past
    y_(i+1).  ValueError: everything the spec can get wrong."""

    def __init__(self, columns, spec):
        if not isinstance(spec, dict) or "functions" not in spec or any(k not in ("functions", "score_mode", "boost_mode") for k in spec):
            raise ValueError("a boost is a dict with \"functions\" and optionally \"score_mode\" / \"boost_mode\"")
        fns = spec["functions"]
        if isinstance(fns, dict):
            fns = [fns]
        if not isinstance(fns, (list, tuple)) or not (1 <= len(fns) <= _capi.SRX_BOOST_MAX_CLAUSES):
            raise ValueError(f"a boost takes 1 to {_capi.SRX_BOOST_MAX_CLAUSES} functions")
        sm, bm = spec.get("score_mode", "multiply"), spec.get("boost_mode", "multiply")
        if not isinstance(sm, str) or sm not in SCORE_MODES:
            raise ValueError(f"score_mode must be one of {', '.join(SCORE_MODES)}, got {sm!r}")
        if not isinstance(bm, str) or bm not in BOOST_MODES:
            raise ValueError(f"boost_mode must be one of {', '.join(BOOST_MODES)}, got {bm!r}")
        self.score_mode_name, self.boost_mode_name = sm, bm
        self.score_mode, self.boost_mode = SCORE_MODES[sm], BOOST_MODES[bm]
        self.columns = columns
        self.functions: List[BoostFunction] = []
        for i, fn in enumerate(fns):
            if not isinstance(fn, dict) or len(fn) != 1 or next(iter(fn)) not in FUNCTION_KINDS or not isinstance(next(iter(fn.values())), dict):
                raise ValueError(f"function {i} must be a dict with one of the keys {', '.join(FUNCTION_KINDS)} and a dict under it")
            kind, body = next(iter(fn.items()))
            self.functions.append(getattr(self, "_" + kind)(body, f"function {i} ({kind})"))
        self.names: List[str] = []
        for f in self.functions:
            if f.field not in self.names:
                self.names.append(f.field)
        self.clauses = np.zeros(len(self.functions), dtype=CLAUSE_DTYPE)
        tables, at = [], 0
        for i, f in enumerate(self.functions):
            self.clauses[i] = (self.names.index(f.field), _capi.SRX_BOOST_ABS if f.abs else 0, f.origin, f.inv_step, f.weight, f.missing, at,
                               len(f.knots) - 1, 0)
            tables.append(f.knots)
            at += len(f.knots)
        if at > _capi.SRX_BOOST_MAX_KNOTS:
            raise ValueError(f"the functions hold {at} knots: a boost takes at most 2^24")
        self.knots = np.ascontiguousarray(np.concatenate(tables), dtype=np.float32)
        self.max_dev = [f.max_dev for f in self.functions]
        self.F_lo, self.F_hi = self._bounds()

    # -- the three kinds ------------------------------------------------------------------------------------------------------------
    def _column(self, body, keys, what):
        bad = [k for k in body if k not in keys]
        if bad:
            raise ValueError(f"{what}: unknown keys {bad}")
        name = body.get("field")
        if not isinstance(name, str) or name not in self.columns:
            raise ValueError(f"{what}: unknown field {name!r}")
        col = self.columns[name]
        if col.kind == "set":
            raise ValueError(f"{what}: {name!r} is a set column: a label set is no number to boost by")
        return name, col, _f32(body.get("weight", 1.0), f"{what}: weight"), _f32(body.get("missing", 1.0), f"{what}: missing")

    def _decay(self, body, what):
        name, col, weight, missing = self._column(body, _DECAY_KEYS, what)
        for k in ("origin", "scale"):
            if k not in body:
                raise ValueError(f"{what}: {k} is required")
        scale, offset = _finite(body["scale"], f"{what}: scale"), _finite(body.get("offset", 0), f"{what}: offset")
        decay, tail = _finite(body.get("decay", 0.5), f"{what}: decay"), _finite(body.get("tail", 1e-3), f"{what}: tail")
        kind = body.get("kind", "gauss")
        if kind not in DECAY_KINDS:
            raise ValueError(f"{what}: kind must be one of {', '.join(DECAY_KINDS)}, got {kind!r}")
        if not scale > 0 or offset < 0 or not (0 < decay < 1) or not (0 < tail < 1):
            raise ValueError(f"{what}: needs scale > 0, offset >= 0, 0 < decay < 1 and 0 < tail < 1")
        n_seg = _segments(body.get("segments", 256), f"{what}: segments")
        origin, _ = _origin_for(col, body["origin"], f"{what}: origin")
        reach = offset + decay_reach(kind, scale, decay, tail)
        inv = _inv_step(reach / n_seg, what)
        knots, dev = _sample(lambda x: decay_value(kind, np.maximum(0.0, x - offset), scale, decay), inv, n_seg, what)
        return BoostFunction(name, True, origin, inv, knots, weight, missing, dev)

    def _field_value(self, body, what):
        name, col, weight, missing = self._column(body, _VALUE_KEYS, what)
        for k in ("lo", "hi"):
            if k not in body:
                raise ValueError(f"{what}: {k} is required")
        modifier = body.get("modifier", "none")
        if not isinstance(modifier, str) or modifier not in MODIFIERS:
            raise ValueError(f"{what}: modifier must be one of {', '.join(MODIFIERS)}, got {modifier!r}")
        factor = _finite(body.get("factor", 1.0), f"{what}: factor")
        n_seg = _segments(body.get("segments", 1 if modifier == "none" else 256), f"{what}: segments")
        origin, lo = _origin_for(col, body["lo"], f"{what}: lo")
        hi = _finite(body["hi"], f"{what}: hi")
        if not hi > lo:
            raise ValueError(f"{what}: needs hi > lo")
        inv = _inv_step((hi - lo) / n_seg, what)
        knots, dev = _sample(lambda x: MODIFIERS[modifier](factor * (lo + x)), inv, n_seg, what)
        return BoostFunction(name, False, origin, inv, knots, weight, missing, dev)

    def _curve(self, body, what):
        name, col, weight, missing = self._column(body, _CURVE_KEYS, what)
        for k in ("origin", "step", "knots"):
            if k not in body:
                raise ValueError(f"{what}: {k} is required")
        origin, _ = _origin_for(col, body["origin"], f"{what}: origin")
        inv = _inv_step(_finite(body["step"], f"{what}: step"), what)
        given = body["knots"]
        if isinstance(given, (str, bytes)) or not hasattr(given, "__len__") or not (2 <= len(given) <= _capi.SRX_BOOST_MAX_KNOTS):
            raise ValueError(f"{what}: knots must be a sequence of 2 to 2^24 numbers")
        knots = np.asarray([_f32(y, f"{what}: a knot") for y in given], dtype=np.float32)
        if not isinstance(body.get("abs", False), (bool, np.bool_)):
            raise ValueError(f"{what}: abs must be a bool")
        return BoostFunction(name, bool(body.get("abs", False)), origin, inv, knots, weight, missing, None)

    # -- bounds ---------------------------------------------------------------------------------------------------------------------
    def _bounds(self):
        lo = hi = None
        with np.errstate(all="ignore"):
            for f in self.functions:
                y = f.knots
                reach = (y[:-1] + (y[1:] - y[:-1]).astype(np.float32)).astype(np.float32)  # what a lerp can round to at most
                ext = np.concatenate([y, reach, np.asarray([f.missing], dtype=np.float32)])
                a, b = np.float32(f.weight * ext.min()), np.float32(f.weight * ext.max())
                g_lo, g_hi = (a, b) if a <= b else (b, a)
                if lo is None:
                    lo, hi = g_lo, g_hi
                elif self.score_mode == _capi.SRX_BOOST_SCORE_MULTIPLY:
                    p = [np.float32(u * v) for u in (lo, hi) for v in (g_lo, g_hi)]
                    lo, hi = min(p), max(p)
                elif self.score_mode == _capi.SRX_BOOST_SCORE_SUM:
                    lo, hi = np.float32(lo + g_lo), np.float32(hi + g_hi)
                elif self.score_mode == _capi.SRX_BOOST_SCORE_MAX:
                    lo, hi = max(lo, g_lo), max(hi, g_hi)
                else:
                    lo, hi = min(lo, g_lo), min(hi, g_hi)
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("the boost overflows float32: its functions' weights and values multiply or add up beyond the float range")
        return np.float32(lo), np.float32(hi)


def check_clause_arrays(types, clauses: np.ndarray, knots: np.ndarray) -> None:
    """What the device does not check of host arrays: ``clauses`` the 40-byte records, every ``col`` in [0, len(types)) and no SET64
    column, ``n_seg`` >= 1 and ``knot0`` / ``n_seg`` inside ``knots``, ``inv_step`` finite and positive, finite knots, weights and
    ``missing``.  Raises ValueError."""
    if not isinstance(clauses, np.ndarray) or clauses.dtype != CLAUSE_DTYPE or clauses.ndim != 1:
        raise ValueError("clauses must be a 1-D array of boost.CLAUSE_DTYPE records (40 bytes each)")
    if not (1 <= len(clauses) <= _capi.SRX_BOOST_MAX_CLAUSES):
        raise ValueError(f"a boost takes 1 to {_capi.SRX_BOOST_MAX_CLAUSES} clauses, got {len(clauses)}")
    knots = np.asarray(knots)
    if knots.dtype != np.float32 or knots.ndim != 1 or not (2 <= len(knots) <= _capi.SRX_BOOST_MAX_KNOTS):
        raise ValueError("knots must be a float32 array of 2 to 2^24 entries")
    if not np.isfinite(knots).all():
        raise ValueError("knots must be finite")
    if any(t == _capi.SRX_FIELD_SET64 for t in types):
        raise ValueError("a set column is no number to boost by")
    for i, c in enumerate(clauses):
        if not (0 <= int(c["col"]) < len(types)):
            raise ValueError(f"clause {i}: col {int(c['col'])} outside [0, {len(types)})")
        if int(c["n_seg"]) < 1 or int(c["knot0"]) < 0 or int(c["knot0"]) + int(c["n_seg"]) >= len(knots):
            raise ValueError(f"clause {i}: its knots [{int(c['knot0'])}, {int(c['knot0'])} + {int(c['n_seg'])}] lie outside the {len(knots)} knots")
        if not (np.isfinite(c["inv_step"]) and c["inv_step"] > 0):
            raise ValueError(f"clause {i}: inv_step must be finite and positive")
        if not (np.isfinite(c["weight"]) and np.isfinite(c["missing"])):
            raise ValueError(f"clause {i}: weight and missing must be finite")


class BoostFn:
    """The ``boost_fn`` of :func:`boost_deep` over a :class:`~.fields.FieldTable`: ``fn(doc, score, count, kk, carry=None)`` ->
    ``(doc [nq, kk], score [nq, kk], count [nq])`` with the contract of ``srx_boost_topk``; ``boost_mode`` ("multiply", "sum",
    "replace"), ``F_lo`` and ``F_hi`` are what the paging bounds an unseen doc with.  The clause records and the knots go to the
    device once."""

    def __init__(self, table, resolved: BoostResolver):
        import torch
        self.table, self.names = table, list(resolved.names)
        self.boost_mode, self.F_lo, self.F_hi = resolved.boost_mode_name, resolved.F_lo, resolved.F_hi
        self.score_mode_id, self.boost_mode_id = resolved.score_mode, resolved.boost_mode
        self.clauses = torch.as_tensor(resolved.clauses.view(np.uint8).reshape(-1, CLAUSE_DTYPE.itemsize).copy(), device=table.device)
        self.knots = torch.as_tensor(resolved.knots, device=table.device)

    def __call__(self, doc, score, count, kk, carry=None, want_pos: bool = False):
        return self.table.boost_device(self.names, self.clauses, self.knots, self.score_mode_id, self.boost_mode_id, doc, score, count, kk,
                                       carry=carry, want_pos=want_pos)


def boost_deep(search_fn, boost_fn, q_ptr, q_term, q_weight, k: int, first: int, page: int = 1024, max_depth: Optional[int] = None):
    """The top ``k`` of the BOOSTED complete ranking, exact, on top of a search limited to ``page`` rows per call.
    ``search_fn(q_ptr, q_term, q_weight, kk, after=None | (doc i32[nq], score f32[nq]))`` as :func:`~.backend.collapse_deep` takes it;
    ``boost_fn(doc [nq, m], score [nq, m], count [nq] | None, kk, carry=None | (doc [nq, kc], score [nq, kc], count [nq])) -> (doc
    [nq, kk], score [nq, kk], count [nq])`` with the contract of ``srx_boost_topk`` and the attributes ``boost_mode``, ``F_lo``,
    ``F_hi`` (:class:`BoostFn`); torch tensors throughout.

    Page 1 (``first`` rows) is boosted to ``k`` rows.  After every page a query is DONE if the page came back short (its ranking is
    exhausted), or if it holds ``k`` rows and ``bound(s_last) < its k-th boosted score``, strictly: every unseen doc has a raw score
    in (0, s_last] and an F in [F_lo, F_hi], so its boosted score is at most ``fl(s_last * F_hi)`` (MULTIPLY, F_lo >= 0) or
    ``fl(s_last + F_hi)`` (SUM) -- rounding is monotone.  On equality it reads on: an unseen doc with a lower id could tie.
    Otherwise the next page -- the rows ranked strictly after its last row -- goes in as candidates with the kept ``k`` rows as the
    carry, whose scores are final.  A finished query's cursor is score 0: nothing ranks after it, its page is empty and its kept
    rows stay.  One synchronisation per page.

    The raw scores must be > 0 (the sparse search guarantees it).  ValueError: ``boost_mode`` "replace" (no bound exists: use
    ``search_sorted``), a negative ``F_lo`` under "multiply" (an unseen doc's raw score then bounds nothing).  ``max_depth`` stops
    after that many rows of the ranking; the result is then the boosted top ``k`` OF THE ROWS READ."""
    import torch
    mode = boost_fn.boost_mode
    if mode == "replace":
        raise ValueError("boost_mode \"replace\" has no bound on an unseen doc: the exact door refuses it (search_sorted orders by a field alone)")
    if mode not in ("multiply", "sum"):
        raise ValueError(f"unknown boost_mode {mode!r}")
    if mode == "multiply" and not float(boost_fn.F_lo) >= 0.0:
        raise ValueError(f"boost_mode \"multiply\" with a factor that can be negative (F_lo = {float(boost_fn.F_lo)!r}) has no bound on an "
                         "unseen doc: the exact door refuses it")
    k = int(k)
    f_hi = float(boost_fn.F_hi)

    def bound(s_last):  # fp32, one rounding: what the device computes for (s_last, F_hi)
        hi = torch.full_like(s_last, f_hi)
        return s_last * hi if mode == "multiply" else s_last + hi

    def reduce(d, s, c, kept, kk):  # the kept rows are the carry: their scores are final
        return boost_fn(d, s, c, kk, carry=None if kept is None else (kept[0].contiguous(), kept[1].contiguous(), kept[2]))

    def unfinished(d, s, c, kk, ks, kc):
        full = c == kk
        settled = (kc == k) & (bound(s[:, kk - 1]) < ks[:, k - 1])
        return full & ~settled

    return deep_reduce(search_fn, reduce, unfinished, q_ptr, q_term, q_weight, k, first, page, max_depth)
