"""Relevance feedback without a GPU: the twelfth header and its symbol table, every refusal of the entry point (none reaches a
device), the row order of the forward index against ``np.lexsort``, the restatement (tests/feedback_ref.py) on three docs worked by
hand, every ``ValueError`` of the Python doors and the mirrors with the new keywords not given."""
import ctypes
import inspect
import json
import math
import os
import re
import tempfile

import numpy as np
import pytest
import torch

import feedback_ref
import sparse_rx
from feedback_ref import BY_SCORE, RAW, RM, UNIFORM
from sparse_rx import _capi, feedback
from sparse_rx.backend import ExpandSpec, SparseBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(20)]  # aligned addresses, never dereferenced
F32 = np.float32


def test_twelfth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "ext", "sparse_rx_feedback.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef SPARSE_RX_FEEDBACK_H")[1]))
    assert declared == set(_capi.FEEDBACK_SYMBOLS) == {"srx_feedback_workspace_bytes", "srx_feedback_expand"}
    assert '#include "sparse_rx.h"' in hdr
    others = (_capi.SYMBOLS, _capi.RESCORE_SYMBOLS, _capi.QUANT_SYMBOLS, _capi.FILTER_SYMBOLS, _capi.HALF_SYMBOLS, _capi.MMR_SYMBOLS,
              _capi.TERMS_SYMBOLS, _capi.MAXSIM_SYMBOLS, _capi.FIELDS_SYMBOLS, _capi.COLLAPSE_SYMBOLS, _capi.FACET_SYMBOLS)
    assert [len(t) for t in others] == [35, 4, 4, 8, 5, 3, 2, 3, 1, 1, 2]
    for other in others:
        assert not set(_capi.FEEDBACK_SYMBOLS) & set(other)
    assert sum(len(t) for t in others) + len(_capi.FEEDBACK_SYMBOLS) == 70
    inc = os.path.join(ROOT, "include")
    assert len([f for f in os.listdir(inc) if f.endswith(".h")]) == 11 and os.listdir(os.path.join(inc, "ext")) == ["sparse_rx_feedback.h"]
    assert "feedback.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "ext", "sparse_rx_feedback.h") in _capi._deps()
    assert "include/ext/sparse_rx_feedback.h" in open(os.path.join(ROOT, "__graft_entry__.py")).read().split('"""')[1]
    L = _capi.lib()
    assert L.srx_version() == 301
    for name, (res, args) in _capi.FEEDBACK_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    for name, value in (("SRX_FEEDBACK_MAX_DOCS", 32), ("SRX_FEEDBACK_MAX_ENTRIES", 4096), ("SRX_FEEDBACK_MAX_TERMS", 128), ("SRX_FEEDBACK_MAX_QTERMS", 128)):
        assert re.search(rf"#define {name}\s+{value}\b", hdr) and getattr(_capi, name) == value == getattr(feedback_ref, name.split("_", 2)[2])
    for name, value in (("SRX_FB_BY_SCORE", 0), ("SRX_FB_UNIFORM", 1), ("SRX_FB_RM", 0), ("SRX_FB_RAW", 1)):
        assert re.search(rf"\b{name} = {value}\b", hdr) and getattr(_capi, name) == value == getattr(feedback_ref, name.split("_", 2)[2])
    D, Q = _capi.ForwardDesc, _capi.FeedbackParams
    assert ctypes.sizeof(D) == 64 and [getattr(D, n).offset for n in ("device", "reserved", "n_docs", "vocab", "doc_base", "row_ptr", "term", "value", "doc_len")] \
        == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    assert ctypes.sizeof(Q) == 28 and [getattr(Q, n).offset for n in ("fb_docs", "row_cap", "n_terms", "doc_weight", "term_weight", "alpha", "beta")] \
        == [0, 4, 8, 12, 16, 20, 24]
    # the struct declarations of the header, field by field
    for struct, cls in (("srx_forward_desc", D), ("srx_feedback_params", Q)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1 + decl.strip().startswith("const"))[-1].split(",")]
        assert names == [n for n, _ in cls._fields_], struct
    assert sparse_rx.ForwardIndex is feedback.ForwardIndex and "ForwardIndex" in sparse_rx.__all__


# ---- every refusal ------------------------------------------------------------------------------------------------------------------
def _refused(rc, word, code=-1):
    msg = _capi.lib().srx_last_error()
    assert rc == code and word.encode() in msg and b"srx_feedback_expand:" in msg, (rc, msg, word)


def _desc(**kw):
    d = dict(device=0, reserved=0, n_docs=1000, vocab=500, doc_base=0, row_ptr=P[0], term=P[1], value=P[2], doc_len=P[3])
    return ctypes.pointer(_capi.ForwardDesc(**{**d, **kw}))


def _par(**kw):
    d = dict(fb_docs=10, row_cap=20, n_terms=10, doc_weight=0, term_weight=0, alpha=0.5, beta=0.5)
    return ctypes.pointer(_capi.FeedbackParams(**{**d, **kw}))


def test_refusals():
    L = _capi.lib()
    ws = int(L.srx_feedback_workspace_bytes(3))
    assert ws >= 3 * (256 * 8 + 4) and L.srx_feedback_workspace_bytes(0) == 0 and L.srx_feedback_workspace_bytes(-1) == -1
    ok = dict(fwd=_desc(), par=_par(), gain=P[4], q_ptr=P[5], q_term=P[6], q_weight=P[7], nq=3, q_nnz=12, fb_doc=P[8], fb_score=P[9], fb_count=P[10], m=40,
              out_ptr=P[11], out_term=P[12], out_weight=P[13], cap=42, flag=P[14], ws=P[15], ws_bytes=ws, stream=None)
    call = lambda **kw: L.srx_feedback_expand(*{**ok, **kw}.values())
    _refused(call(fwd=None), "null forward descriptor")
    _refused(call(par=None), "null params")
    for n in (0, -1, 2 ** 31 - 1, 2 ** 40):
        _refused(call(fwd=_desc(n_docs=n)), "n_docs must be in [1, 2^31 - 2]")
    for v in (0, -1, 2 ** 26 + 1, 2 ** 40):
        _refused(call(fwd=_desc(vocab=v)), "vocab must be in [1, 2^26]")
    _refused(call(fwd=_desc(doc_base=-1)), "negative doc_base")
    for base in (2 ** 31 - 1 - 1000, 2 ** 40):
        _refused(call(fwd=_desc(doc_base=base)), "doc_base + n_docs must be below 2^31 - 1")
    for r in (0, -1, 33, 2 ** 20):
        _refused(call(par=_par(fb_docs=r)), "fb_docs must be in [1, 32]")
    for c in (0, -1):
        _refused(call(par=_par(row_cap=c)), "row_cap must be >= 1")
    for r, c in ((32, 129), (10, 410), (1, 4097), (32, 2 ** 31 - 1)):
        _refused(call(par=_par(fb_docs=r, row_cap=c)), "fb_docs * row_cap must not exceed 4096")
    for n in (0, -1, 129):
        _refused(call(par=_par(n_terms=n)), "n_terms must be in [1, 128]")
    for mode in (-1, 2, 99):
        _refused(call(par=_par(doc_weight=mode)), "unknown doc_weight")
        _refused(call(par=_par(term_weight=mode)), "unknown term_weight")
    _refused(call(fwd=_desc(doc_len=None)), "SRX_FB_RM needs doc_len")
    for bad in (-0.5, math.nan, math.inf, -math.inf):
        _refused(call(par=_par(alpha=bad)), "alpha and beta must be finite and >= 0")
        _refused(call(par=_par(beta=bad)), "alpha and beta must be finite and >= 0")
    _refused(call(par=_par(alpha=0.0, beta=0.0)), "alpha and beta are both 0")
    _refused(call(par=_par(alpha=-0.0, beta=0.0)), "alpha and beta are both 0")
    _refused(call(nq=-1), "nq < 0")
    for m in (0, -1):
        _refused(call(m=m), "m must be >= 1")
    _refused(call(nq=2 ** 16, m=2 ** 15, cap=2 ** 40), "nq * m")
    for n in (-1, 2 ** 31):
        _refused(call(q_nnz=n, cap=2 ** 40), "q_nnz must be in [0, 2^31 - 1]")
    _refused(call(q_nnz=2 ** 31 - 30, cap=2 ** 40), "q_nnz + nq * n_terms must not exceed 2^31 - 1")
    for cap in (41, 0, -1):
        _refused(call(cap=cap), "out_capacity is below q_nnz + nq * n_terms")
    for name in ("row_ptr", "term", "value"):
        _refused(call(fwd=_desc(**{name: None})), "null row_ptr / term / value")
    for name in ("q_ptr", "q_term", "q_weight"):
        _refused(call(**{name: None}), "null q_ptr / q_term / q_weight")
    for name in ("fb_doc", "fb_score"):
        _refused(call(**{name: None}), "null fb_doc / fb_score")
    for name in ("out_ptr", "out_term", "out_weight", "flag"):
        _refused(call(**{name: None}), "null out_ptr / out_term / out_weight / flag")
    _refused(call(ws=None), "workspace too small", code=-3)
    _refused(call(ws_bytes=ws - 1), "workspace too small", code=-3)
    # the limits themselves pass the checks (they are refused for the workspace, the last check before the device)
    for kw in (dict(par=_par(fb_docs=32, row_cap=128, n_terms=128), cap=12 + 3 * 128), dict(par=_par(fb_docs=1, row_cap=4096)), dict(fwd=_desc(vocab=2 ** 26)),
               dict(fwd=_desc(n_docs=2 ** 31 - 2)), dict(fwd=_desc(doc_base=2 ** 31 - 2 - 1000)), dict(par=_par(alpha=0.0, beta=1.0)),
               dict(par=_par(alpha=3.0, beta=0.0)), dict(par=_par(term_weight=1), fwd=_desc(doc_len=None)), dict(par=_par(doc_weight=1), fb_score=None),
               dict(q_nnz=0, cap=30, q_term=None, q_weight=None), dict(gain=None), dict(fb_count=None)):
        _refused(call(ws_bytes=0, **kw), "workspace too small", code=-3)
    # nothing to do: no launch, whatever the pointers are; the checks still come first
    none = dict(q_ptr=None, q_term=None, q_weight=None, fb_doc=None, fb_score=None, out_ptr=None, out_term=None, out_weight=None, flag=None, ws=None, ws_bytes=0)
    assert call(nq=0, q_nnz=0, cap=0, **none) == 0 and call(nq=0) == 0 and call(nq=0, fwd=_desc(row_ptr=None, term=None, value=None), **none) == 0
    _refused(call(nq=0, par=_par(fb_docs=33)), "fb_docs")
    _refused(call(nq=0, m=0), "m must be >= 1")
    _refused(call(nq=0, cap=11), "out_capacity")


# ---- the row order -------------------------------------------------------------------------------------------------------------------
def test_row_order_against_lexsort():
    rng = np.random.default_rng(3)
    n_docs, vocab = 40, 30
    rows, terms = [], []
    for d in range(n_docs):
        t = np.sort(rng.choice(vocab, int(rng.integers(0, 12)), replace=False))
        rows += [d] * len(t)
        terms += t.tolist()
    row, term = np.asarray(rows, np.int32), np.asarray(terms, np.int32)
    value = rng.integers(1, 4, len(term)).astype(np.float32)  # small integers: many equal keys
    idf = rng.choice(np.asarray([-1.5, -0.0, 0.0, 0.5, 1.0, 2.0], np.float32), vocab)  # negative idfs, and both zeros
    idf[:4] = [0.0, -0.0, 0.0, -0.0]
    key = (value * idf[term]).astype(np.float32)
    assert (np.signbit(key) & (key == 0)).any() and (~np.signbit(key) & (key == 0)).any() and (key < 0).any()
    want = np.lexsort((term, -key, row))
    # fed in any order, the permutation is lexsort's: -0 and +0 tie and go by term
    for shuffle in (np.arange(len(term)), rng.permutation(len(term))):
        got = feedback.forward_order(torch, torch.from_numpy(row[shuffle]), torch.from_numpy(term[shuffle]), torch.from_numpy(value[shuffle]),
                                     torch.from_numpy(idf)).numpy()
        assert np.array_equal(shuffle[got], want)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n_docs))]).astype(np.int64)
    rp, t2, v2, longest = feedback_ref.forward_rows(indptr, term, value, idf)
    assert np.array_equal(t2, term[want]) and np.array_equal(v2, value[want]) and np.array_equal(rp, indptr) and longest == np.diff(indptr).max()
    # one row by hand: keys 2 * 1 = 2, 1 * -1.5 = -1.5, 3 * -0 = -0, 1 * 0 = 0, 1 * 2 = 2
    idf = np.asarray([1.0, -1.5, -0.0, 0.0, 2.0], np.float32)
    _, t, v, _ = feedback_ref.forward_rows([0, 5], [0, 1, 2, 3, 4], [2, 1, 3, 1, 1], idf)
    assert t.tolist() == [0, 4, 2, 3, 1] and v.tolist() == [2, 1, 3, 1, 1]


# ---- the restatement by hand -------------------------------------------------------------------------------------------------------
def _hand():
    """Three docs, doc_base 100.  Rows (term: value), doc_len: doc 0 = {1: 2, 3: 2} len 4; doc 1 = {3: 1, 5: 4, 7: 3} len 8;
    doc 2 = {1: 1, 9: 1} len 2."""
    return dict(row_ptr=np.asarray([0, 2, 5, 7], np.int64), term=np.asarray([1, 3, 5, 7, 3, 1, 9], np.int32),
                value=np.asarray([2, 2, 4, 3, 1, 1, 1], np.float32), doc_len=np.asarray([4, 8, 2], np.float32), n_docs=3, doc_base=100)


def _expand(q, fb, fb_docs=3, row_cap=3, n_terms=2, dw=BY_SCORE, tw=RM, alpha=0.5, beta=0.5, gain=None, **kw):
    h = {**_hand(), **kw}
    q_ptr = np.concatenate([[0], np.cumsum([len(r) for r in q])]).astype(np.int32)
    q_term = np.asarray([t for r in q for t, _ in r], np.int32)
    q_weight = np.asarray([w for r in q for _, w in r], np.float32)
    doc, score, count = fb
    p, t, w, flag = feedback_ref.expand(h["row_ptr"], h["term"], h["value"], h["doc_len"], h["n_docs"], h["doc_base"], fb_docs, row_cap, n_terms, dw, tw,
                                        alpha, beta, gain, q_ptr, q_term, q_weight, np.asarray(doc, np.int32), np.asarray(score, np.float32), count)
    return [list(zip(t[p[i]: p[i + 1]].tolist(), w[p[i]: p[i + 1]].tolist())) for i in range(len(q))], flag


def test_restatement_by_hand():
    # query {1: 1, 3: 3}; docs 0 and 1 with the scores 3 and 1: a = 3/4, 1/4.
    # fb(1) = .75 * 2/4 = .375; fb(3) = .75 * 2/4 + .25 * 1/8 = .40625; fb(5) = .25 * 4/8 = .125; fb(7) = .25 * 3/8 = .09375
    # n_terms 2: 3 and 1 are selected, F = .78125; Q = 4.  w(1) = .5 * 1/4 + .5 * .375 / .78125 = .365; w(3) = .5 * 3/4 + .5 * .52 = .635
    q = [[(1, 1.0), (3, 3.0)]]
    rows, flag = _expand(q, ([[100, 101, 102]], [[3.0, 1.0, 0.0]], None))
    assert flag == 0 and rows == [[(1, float(F32(0.125) + F32(0.5) * (F32(0.375) / F32(0.78125)))), (3, float(F32(0.375) + F32(0.5) * (F32(0.40625) / F32(0.78125))))]]
    assert abs(rows[0][0][1] - 0.365) < 1e-7 and abs(rows[0][1][1] - 0.635) < 1e-7
    # n_terms 3 adds 5: F = .90625, and 5 gets B alone
    rows, _ = _expand(q, ([[100, 101, 102]], [[3.0, 1.0, 0.0]], None), n_terms=3)
    assert [t for t, _ in rows[0]] == [1, 3, 5] and rows[0][2][1] == float(F32(0.5) * (F32(0.125) / F32(0.90625)))
    # a gain that bans 3 and doubles 7: candidates 1 (.375), 5 (.125), 7 (.1875) -> 1 and 7; 3 stays as a query term with A alone
    rows, _ = _expand(q, ([[100, 101, 102]], [[3.0, 1.0, 0.0]], None), gain=np.asarray([1, 1, 1, 0, 1, 1, 1, 2, 1, 1], np.float32))
    assert [t for t, _ in rows[0]] == [1, 3, 7] and rows[0][1][1] == 0.375 and rows[0][2][1] == float(F32(0.5) * (F32(0.09375) / F32(0.46875)))
    # row_cap 1: the first entry of every row only -- doc 0: term 1 (.375), doc 1: term 5 (.125); F = .5; 3 has A alone
    rows, _ = _expand(q, ([[100, 101, 102]], [[3.0, 1.0, 0.0]], None), row_cap=1)
    assert rows[0] == [(1, 0.125 + 0.5 * 0.75), (3, 0.375), (5, 0.5 * 0.25)]
    # UNIFORM + RAW over all three docs: a = 1/3 each; fb(1) = 2/3 + 1/3 (in that order), fb(3) = 2/3 + 1/3, fb(5) = 4/3, fb(7) = 1, fb(9) = 1/3
    third = F32(1) / F32(3)
    rows, _ = _expand([[]], ([[100, 101, 102]], [[0.0, 0.0, 0.0]], None), dw=UNIFORM, tw=RAW, n_terms=3, alpha=0.0, beta=1.0)
    fb1, fb5 = F32(third * F32(2)) + third, third * F32(4)
    assert [t for t, _ in rows[0]] == [1, 3, 5]  # 5 first by value; 1 and 3 tie at 1 and beat 7 by term id
    assert fb1 == F32(1) and rows[0][2][1] == float(fb5 / F32(F32(F32(1) + F32(1)) + fb5))
    # the liveness rules: count, the doc range, the score; a doc listed twice counts twice; an empty query and no used doc
    rows, _ = _expand(q + [[]] + q, ([[100, 101, 102], [99, 103, -1], [100, 100, 101]], [[3.0, 1.0, 5.0], [1.0, 1.0, 1.0], [1.0, 1.0, np.nan]], [1, 3, 3]))
    assert [t for t, _ in rows[0]] == [1, 3] and rows[0][0][1] == float(F32(0.125) + F32(0.5) * (F32(0.5) / F32(1.0)))  # doc 0 alone: a = 1
    assert rows[1] == [] and rows[2] == rows[0]  # a = 1/2 twice: fb(1) = .25 + .25
    rows, _ = _expand(q, ([[100, 101, 102]], [[0.0, -1.0, np.inf]], None))
    assert rows[0] == [(1, 0.125), (3, 0.375)]  # no used doc: the normalised query at alpha
    # alpha 0: the unselected query term 3 vanishes under a gain that bans it; beta 0: the query alone; Q = 0: no A
    rows, _ = _expand(q, ([[100, 101, 102]], [[3.0, 1.0, 0.0]], None), alpha=0.0, beta=1.0, gain=np.asarray([1, 1, 1, 0, 1, 1, 1, 1, 1, 1], np.float32))
    assert [t for t, _ in rows[0]] == [1, 5]
    rows, _ = _expand(q, ([[100, 101, 102]], [[3.0, 1.0, 0.0]], None), alpha=1.0, beta=0.0)
    assert rows[0] == [(1, 0.25), (3, 0.75)]
    rows, _ = _expand([[(1, 0.0), (8, 0.0)]], ([[100, 101, 102]], [[3.0, 1.0, 0.0]], None))
    assert [t for t, _ in rows[0]] == [1, 3] and rows[0][0][1] == float(F32(0.5) * (F32(0.375) / F32(0.78125)))
    # an over-long query is copied through, order kept, and flags
    long_q = [(200 - i, float(i + 1)) for i in range(129)]
    rows, flag = _expand([long_q] + q, ([[100, 101, 102]] * 2, [[3.0, 1.0, 0.0]] * 2, None))
    assert flag == 1 and rows[0] == long_q and abs(rows[1][0][1] - 0.365) < 1e-7


# ---- the Python doors ---------------------------------------------------------------------------------------------------------------
def test_check_expand_args():
    assert feedback.check_expand_args(5, 10, 0.5) == (5, 10, 0.5, "score") and feedback.check_expand_args(32, 128, 1, "uniform") == (32, 128, 1.0, "uniform")
    assert feedback.check_expand_args(1, 1, 0) == (1, 1, 0.0, "score")
    for bad in (0, -1, 33, 2.5, True):
        with pytest.raises(ValueError, match=r"expand_docs must be in \[1, 32\]"):
            feedback.check_expand_args(bad, 10, 0.5)
    for bad in (0, 129, 1.5):
        with pytest.raises(ValueError, match=r"expand_terms must be in \[1, 128\]"):
            feedback.check_expand_args(5, bad, 0.5)
    for bad in (-0.1, 1.01, math.nan, math.inf):
        with pytest.raises(ValueError, match=r"expand_weight must be in \[0, 1\]"):
            feedback.check_expand_args(5, 10, bad)
    with pytest.raises(ValueError, match="expand_by must be 'score' or 'uniform'"):
        feedback.check_expand_args(5, 10, 0.5, "rank")


def _stub_backend():
    be = SparseBackend("cuda:0", 14)
    be.host = type("Host", (), {"doc_ids": [f"d{i}" for i in range(40)], "vocabulary": {"w": 0}, "n_docs": 40, "vocab_size": 1})()
    be.dev = type("Dev", (), {"close": lambda self: None})()
    be.n_docs_total = 40
    return be


def test_backend_refusals_without_a_forward_index():
    be = _stub_backend()
    assert be.expand_spec(None, expand_terms=0, expand_weight=9, expand_by="x") is None  # not looked at without expand_docs
    with pytest.raises(ValueError, match=r"search\(expand_docs=\.\.\.\) needs the forward index: call enable_feedback\(\) first"):
        be.expand_spec(5)
    with pytest.raises(ValueError, match=r"expand_docs must be in \[1, 32\]"):
        be.expand_spec(33)  # the range comes first
    with pytest.raises(ValueError, match=r"expand_weight must be in \[0, 1\]"):
        be.expand_spec(5, expand_weight=2)
    with pytest.raises(ValueError, match=r"more_like_this\(\.\.\.\) needs the forward index: call enable_feedback\(\) first"):
        be.more_like_this({"q": ["d1"]})
    with pytest.raises(ValueError, match=r"expand_queries\(\.\.\.\) needs the forward index"):
        be.expand_queries({"q": "w"}, {"q": {"d1": 1.0}})
    with pytest.raises(ValueError, match=r"expand_terms must be in \[1, 128\]"):
        be.more_like_this({"q": ["d1"]}, terms=129)
    be.host = be.dev = None
    with pytest.raises(ValueError, match="enable_feedback\\(\\) needs the sparse index"):
        be.enable_feedback()
    # with a forward index (a stub: nothing is launched): the seeds are checked before anything else happens
    be = _stub_backend()
    be._forward = type("Fwd", (), {"close": lambda self: None})()
    spec = be.expand_spec(7, 3, 0.25, "uniform")
    assert isinstance(spec, ExpandSpec) and (spec.docs, spec.terms, spec.weight, spec.by) == (7, 3, 0.25, "uniform")
    with pytest.raises(ValueError, match="at most 32 seeds per query, got 33 for 'q'"):
        be.more_like_this({"q": [f"d{i}" for i in range(33)]})
    with pytest.raises(ValueError, match="unknown doc id 'zz' among the seeds of 'q'"):
        be.more_like_this({"q": ["d1", "zz"]})
    with pytest.raises(ValueError, match="seeds must be a dict"):
        be.more_like_this(["d1"])
    with pytest.raises(ValueError, match=r"seeds\['q'\] must be a sequence of doc ids, not one string"):
        be.more_like_this({"q": "d1"})
    with pytest.raises(ValueError, match="at most 32 results per query"):
        be.expand_queries({"q": "w"}, {"q": {f"d{i}": 1.0 for i in range(33)}})
    with pytest.raises(ValueError, match="unknown doc id 'zz'"):
        be.expand_queries({"q": "w"}, {"q": {"zz": 1.0}})
    assert be.more_like_this({}) == {} and be.expand_queries({}, {}) == {}
    be.close()
    assert be._forward is None  # close() drops it ...
    be._forward = type("Fwd", (), {"close": lambda self: None})()
    be.dev = None
    be.host = type("Host", (), {"n_docs": 0})()
    be._searcher_factory, be._force_sharded = (lambda *a: None), False
    be.sharded = lambda: True
    be.upload("bm25", 1.2, 0.75)
    assert be._forward is None  # ... and so does upload()


def test_forward_index_refusals_on_device_tensors():
    ix = feedback.ForwardIndex(None, None, None, None, 10, 5, 0, 3, torch.device("cpu"))
    i32, f32 = lambda *s: torch.zeros(s, dtype=torch.int32), lambda *s: torch.zeros(s, dtype=torch.float32)
    ok = dict(q_ptr=i32(3), q_term=i32(4), q_weight=f32(4), fb_doc=i32(2, 6), fb_score=f32(2, 6), fb_count=i32(2))
    for kw, word in ((dict(q_ptr=i32(3).long()), "int32 tensors"), (dict(q_weight=f32(4).double()), "float32 tensor"), (dict(fb_doc=i32(3, 6)), r"\[nq, m >= 1\]"),
                     (dict(fb_doc=i32(2, 0)), r"\[nq, m >= 1\]"), (dict(fb_doc=i32(2, 6).long()), r"\[nq, m >= 1\]"), (dict(fb_score=f32(2, 5)), "fb_doc's shape"),
                     (dict(fb_count=i32(3)), r"int32 tensor \[nq\]"), (dict(term_gain=f32(4)), r"float32 tensor \[vocab\]"), (dict(doc_weight="rank"), "doc_weight must be"),
                     (dict(term_weight="tf"), "term_weight 'rm' or 'raw'")):
        with pytest.raises(ValueError, match=word):
            ix.expand_device(**{**ok, **kw}, fb_docs=5)
    assert ix.default_row_cap(10) == 3 and feedback.ForwardIndex(None, None, None, None, 10, 5, 0, 900, torch.device("cpu")).default_row_cap(32) == 128
    # host batches are validated like a search's
    with pytest.raises(ValueError, match="same term twice"):
        ix.expand(np.asarray([0, 2]), np.asarray([1, 1]), np.ones(2, np.float32), np.zeros((1, 3), np.int32), fb_docs=3)
    with pytest.raises(ValueError, match="q_term out of range"):
        ix.expand(np.asarray([0, 1]), np.asarray([5]), np.ones(1, np.float32), np.zeros((1, 3), np.int32), fb_docs=3)
    with pytest.raises(ValueError, match="cand_doc has 2 rows for 1 queries"):
        ix.expand(np.asarray([0, 1]), np.asarray([1]), np.ones(1, np.float32), np.zeros((2, 3), np.int32), fb_docs=3)
    ix.close()
    with pytest.raises(ValueError, match="the forward index is closed"):
        ix.expand_device(**ok, fb_docs=5)
    if not torch.cuda.is_available():
        with pytest.raises(_capi.SparseRxUnavailable, match="ForwardIndex needs a GPU"):
            feedback.ForwardIndex.from_csr([0, 1], [0], [1.0], [1.0])


# ---- the mirrors -------------------------------------------------------------------------------------------------------------------
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


def test_mirrors_take_the_old_path_without_the_keywords(golden_dir, one_rank_group, tmp_path):
    """The fake backend of test_dict_search_cpu.py (the CPU oracle behind the sharding protocol, counting its searches): without
    the new keywords the searches run and cache as before, and give the golden results; the feedback doors refuse a sharded index
    before any search."""
    from test_dict_search_cpu import _Counted
    j = json.load(open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8"))
    q = {qid: j["queries"][qid] for qid in ("q0", "q1", "q2")}
    for make, method in ((lambda f: sparse_rx.RetrievalService(shard_searcher_factory=f, sharded=True), "search_bm25"),
                         (lambda f: sparse_rx.OptimizedBM25Retriever(shard_searcher_factory=f, sharded=True), "search"),
                         (lambda f: sparse_rx.OptimizedRetriever({"type": "bm25"}, shard_searcher_factory=f, sharded=True, cache_dir=str(tmp_path)), "search")):
        f = _Counted()
        o = make(f)
        for door, args in ((o.enable_feedback, ()), (o.more_like_this, ({"q": ["doc1"]},)), (o.expand_queries, (q, {}))):
            with pytest.raises(ValueError, match="not built"):
                door(*args)
        (o.build_bm25_index if method == "search_bm25" else o.build_index_from_corpus)(j["corpus"])
        search = getattr(o, method)
        r = search(q, top_k=10)
        assert f.take() == [(3, 10)] and len(o.query_cache) == 3 and all(r[qid] for qid in q)
        assert search(q, top_k=10, expand_docs=None, expand_terms=0, expand_weight=7.0, expand_by="nothing") == r  # None: the others are not looked at
        assert f.take() == [] and len(o.query_cache) == 3  # ... and the call was served from the cache
        with pytest.raises(ValueError, match=r"expand_docs must be in \[1, 32\]"):
            search(q, top_k=10, expand_docs=0)
        with pytest.raises(ValueError, match=r"expand_weight must be in \[0, 1\]"):
            search(q, top_k=10, expand_docs=5, expand_weight=1.5)
        with pytest.raises(ValueError, match=r"\(expand_docs=\.\.\.\) needs the whole index on one GPU"):
            search(q, top_k=10, expand_docs=5)
        with pytest.raises(ValueError, match="needs the whole index on one GPU"):
            o.more_like_this({"q": ["doc1"]})
        with pytest.raises(ValueError, match="needs the whole index on one GPU"):
            o.expand_queries(q, r)
        with pytest.raises(ValueError, match="enable_feedback\\(\\) needs the sparse index|whole index on one GPU"):
            o.enable_feedback()
        assert f.take() == [] and search(q, top_k=10) == r
        o.close()


def test_doors_and_their_defaults():
    for cls, name in ((sparse_rx.RetrievalService, "search_bm25"), (sparse_rx.OptimizedBM25Retriever, "search"), (sparse_rx.OptimizedRetriever, "search")):
        sig = inspect.signature(getattr(cls, name)).parameters
        want = dict(expand_docs=None, expand_terms=10, expand_weight=0.5, expand_by="score")
        assert {k: sig[k].default for k in want} == want and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
        assert "not comparable" in " ".join(getattr(cls, name).__doc__.lower().split())
        mlt = inspect.signature(cls.more_like_this).parameters
        assert list(mlt)[:5] == ["self", "seeds", "top_k", "terms", "include_seeds"] and (mlt["top_k"].default, mlt["terms"].default, mlt["include_seeds"].default) == (10, 25, False)
        assert {"allowed_docs", "excluded_docs", "must_terms", "any_terms", "must_not_terms", "where"} <= set(mlt)
        assert list(inspect.signature(cls.expand_queries).parameters)[:3] == ["self", "queries", "results"] and callable(cls.enable_feedback)
    for cls in (sparse_rx.HybridRetriever, sparse_rx.ShardedSearcher, sparse_rx.HostBatchPipeline):
        assert not hasattr(cls, "more_like_this") and not hasattr(cls, "enable_feedback") and not hasattr(cls, "expand_queries")
        for name in ("search", "submit"):
            if hasattr(cls, name):
                assert "expand_docs" not in inspect.signature(getattr(cls, name)).parameters
    assert "expand_docs" not in inspect.signature(sparse_rx.RetrievalService.search_hybrid).parameters
    for name in ("from_csr", "expand_device", "expand", "device_bytes", "close"):
        assert callable(getattr(sparse_rx.ForwardIndex, name))
