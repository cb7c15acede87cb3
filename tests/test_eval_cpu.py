"""Ranking evaluation without a GPU: the sixteenth header and its symbol table, every refusal of ``srx_eval_lists`` (none reaches a
device), the fp32 restatement against the float64 one within the bound fp32 rounding gives, cases worked by hand, the Judgments
builders, and the two host halves of the dict door around the restatement."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import eval_ref
import sparse_rx
from sparse_rx import _capi, evaluate as ev
from sparse_rx.backend import SparseIndexViews

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [(i + 1) << 20 for i in range(24)]  # aligned addresses, never dereferenced
U = 2.0 ** -24                          # the unit roundoff of float32

OTHER_TABLES = {"SYMBOLS": 35, "RESCORE_SYMBOLS": 4, "QUANT_SYMBOLS": 4, "FILTER_SYMBOLS": 8, "HALF_SYMBOLS": 5, "MMR_SYMBOLS": 3, "TERMS_SYMBOLS": 2,
                "MAXSIM_SYMBOLS": 3, "FIELDS_SYMBOLS": 1, "COLLAPSE_SYMBOLS": 1, "FACET_SYMBOLS": 2, "FEEDBACK_SYMBOLS": 2, "ORDER_SYMBOLS": 3,
                "BOOST_SYMBOLS": 1, "LTR_SYMBOLS": 2}


def _ks(*ks):
    return (ctypes.c_int32 * max(len(ks), 1))(*ks)


def _lists(L, device=0, j_ptr=P[0], j_doc=P[1], j_grade=P[2], j_ideal=P[3], n_rows=4, nnz=100, gain=P[4], n_gain=5, discount=P[5], rel_level=1,
           cand_doc=P[6], cand_count=P[7], q_row=P[8], nq=3, m=100, ks=None, n_k=2, out=P[9], out_hits=P[10], out_judged=P[11], out_rel=P[12],
           out_mean=P[13], out_n=P[14], workspace=P[15], workspace_bytes=1 << 20, stream=None):
    if ks is None:
        ks = _ks(10, 100)
    return L.srx_eval_lists(device, j_ptr, j_doc, j_grade, j_ideal, n_rows, nnz, gain, n_gain, discount, rel_level, cand_doc, cand_count, q_row, nq, m,
                            ks, n_k, out, out_hits, out_judged, out_rel, out_mean, out_n, workspace, workspace_bytes, stream)


def test_sixteenth_header_and_table():
    hdr = open(os.path.join(ROOT, "include", "eval", "sparse_rx_eval.h")).read()
    declared = set(re.findall(r"\b(srx_[a-z_0-9]+)\s*\(", hdr.split("#ifndef SPARSE_RX_EVAL_H")[1]))
    assert declared == set(_capi.EVAL_SYMBOLS) == {"srx_eval_workspace_bytes", "srx_eval_lists"}
    assert len(OTHER_TABLES) == 15
    for name, size in OTHER_TABLES.items():
        table = getattr(_capi, name)
        assert len(table) == size, name
        assert not set(_capi.EVAL_SYMBOLS) & set(table)
    assert sum(OTHER_TABLES.values()) + len(_capi.EVAL_SYMBOLS) == 78
    assert os.listdir(os.path.join(ROOT, "include", "eval")) == ["sparse_rx_eval.h"]
    assert "eval.hip" in _capi.SOURCES and os.path.join(_capi.INCLUDE_DIR, "eval", "sparse_rx_eval.h") in _capi._deps()
    assert "include/eval/sparse_rx_eval.h" in _capi.__doc__
    L = _capi.lib()
    for name, (res, args) in _capi.EVAL_SYMBOLS.items():
        f = getattr(L, name)  # exported from the same library
        assert f.restype is res and list(f.argtypes) == args, name
    assert len(_capi.EVAL_SYMBOLS["srx_eval_lists"][1]) == len(inspect.signature(_lists).parameters) - 1 == 27
    assert len(_capi.EVAL_SYMBOLS["srx_eval_workspace_bytes"][1]) == 2
    for i, name in enumerate(("NDCG", "AP", "RECALL", "P", "RR", "SUCCESS", "DCG", "IDCG")):
        assert re.search(rf"\bSRX_EVAL_{name} = {i}\b", hdr) and getattr(_capi, f"SRX_EVAL_{name}") == i == getattr(eval_ref, name), name
    # the size constants: the header, the binding, the module and the restatement; the kernel file names the two of the per-query stage
    for name, value, ref in (("SRX_EVAL_METRICS", 8, "METRICS"), ("SRX_EVAL_MAX_M", 2048, "MAX_M"), ("SRX_EVAL_MAX_K", 8, "MAX_K"),
                             ("SRX_EVAL_MAX_GAIN", 32, "MAX_GAIN"), ("SRX_EVAL_WAVE_M", 256, "WAVE_M"), ("SRX_EVAL_LDS_ROW", 1024, "LDS_ROW"),
                             ("SRX_EVAL_MEAN_CHUNK", 1024, "MEAN_CHUNK")):
        assert re.search(rf"#define {name} {value}\b", hdr) and getattr(_capi, name) == value == getattr(eval_ref, ref), name
    assert (ev.WAVE_M, ev.LDS_ROW, ev.MEAN_CHUNK) == (256, 1024, 1024)
    src = open(os.path.join(_capi.CSRC_DIR, "eval.hip")).read().split("#include")[0]
    assert re.search(r"SRX_EVAL_WAVE_M\s+= 256\b", src) and re.search(r"SRX_EVAL_LDS_ROW = 1024\b", src)
    assert sparse_rx.Judgments is ev.Judgments and {"evaluate", "Judgments"} <= set(sparse_rx.__all__)
    # the workspace formula: 8 bytes per (chunk, cutoff, metric) and 8 per chunk
    for nq, n_k in ((0, 1), (1, 1), (1024, 8), (1025, 8), (65536, 4)):
        assert L.srx_eval_workspace_bytes(nq, n_k) == -(-nq // 1024) * (n_k * 64 + 8)
    for nq, n_k in ((-1, 1), (1, 0), (1, 9)):
        assert L.srx_eval_workspace_bytes(nq, n_k) == -1 and L.srx_last_error().startswith(b"srx_eval_workspace_bytes")


def refusals():
    """Every refusal of ``srx_eval_lists``: all return SRX_ERR_INVALID with their message, none touches a device (the pointers are
    never dereferenced); then what passes, on nq == 0.  tests/test_eval_gpu.py runs the same list on the GPU machine."""
    L = _capi.lib()
    null_ks = ctypes.cast(None, ctypes.POINTER(ctypes.c_int32))

    def no(rc, word):
        msg = L.srx_last_error()
        assert rc == -1 and word.encode() in msg and msg.startswith(b"srx_eval_lists"), (rc, msg, word)

    for n in (-1, -5):
        no(_lists(L, n_rows=n), "negative n_rows / nnz")
    no(_lists(L, nnz=-1), "negative n_rows / nnz")
    for name in ("j_ptr", "j_doc", "j_grade", "j_ideal"):
        no(_lists(L, **{name: None}), "null j_ptr / j_doc / j_grade / j_ideal")
    for n in (0, -1, 33):
        no(_lists(L, n_gain=n), "n_gain must be in [1, 32]")
    for name in ("gain", "discount"):
        no(_lists(L, **{name: None}), "null gain / discount")
    for r in (0, -1):
        no(_lists(L, rel_level=r), "rel_level must be >= 1")
    for m in (0, -1, 2049, 2 ** 31 - 1):
        no(_lists(L, m=m), "m must be in [1, 2048]")
    for n in (0, -1, 9):
        no(_lists(L, n_k=n), "n_k must be in [1, 8]")
    no(_lists(L, ks=null_ks), "null ks")
    for ks in ((0, 5), (-3, 5), (1, 0)):
        no(_lists(L, ks=_ks(*ks)), "a cutoff must be >= 1")
    for ks in ((5, 5), (10, 3)):
        no(_lists(L, ks=_ks(*ks)), "strictly ascending")
    no(_lists(L, ks=_ks(1, 2, 3, 3), n_k=4), "strictly ascending")
    no(_lists(L, nq=-1), "nq >= 0 and nq * m <= 2^31 - 1")
    no(_lists(L, nq=2 ** 31 - 1, m=2048), "nq >= 0 and nq * m <= 2^31 - 1")
    no(_lists(L, nq=1 << 20, m=2048), "nq >= 0 and nq * m <= 2^31 - 1")
    for name in ("cand_doc", "out", "out_hits", "out_judged", "out_rel"):
        no(_lists(L, **{name: None}), "null cand_doc / out / out_hits / out_judged / out_rel")
    no(_lists(L, out_mean=None), "out_mean and out_n go together")
    no(_lists(L, out_n=None), "out_mean and out_n go together")
    no(_lists(L, workspace=None), "the means need a workspace")
    no(_lists(L, workspace=P[15] + 4), "the means need a workspace")
    no(_lists(L, workspace_bytes=L.srx_eval_workspace_bytes(3, 2) - 1), "the means need a workspace")
    no(_lists(L, nq=1025, workspace_bytes=L.srx_eval_workspace_bytes(1024, 2)), "the means need a workspace")
    # what passes, on nq == 0 (no launch): the limits, no judged query at all, no count / rows / means
    nothing = dict(nq=0, cand_doc=None, out=None, out_hits=None, out_judged=None, out_rel=None)
    assert _lists(L, **nothing) == 0 and _lists(L, nq=0) == 0
    assert _lists(L, **nothing, n_rows=0, nnz=0, j_ptr=None, j_doc=None, j_grade=None, j_ideal=None) == 0
    assert _lists(L, **nothing, n_gain=1, m=1, ks=_ks(1), n_k=1, cand_count=None, q_row=None) == 0
    assert _lists(L, **nothing, n_gain=32, m=2048, ks=_ks(1, 2, 3, 4, 5, 6, 7, 2 ** 31 - 1), n_k=8, rel_level=2 ** 31 - 1) == 0
    assert _lists(L, **nothing, out_mean=None, out_n=None, workspace=None, workspace_bytes=0) == 0
    assert _lists(L, **nothing, workspace=None, workspace_bytes=0) == 0  # no query: no workspace needed


def test_entry_point_refusals():
    refusals()


# ---- the two restatements ------------------------------------------------------------------------------------------------------------
def random_case(rng, nq, m, n_rows, max_row, n_docs, grades=(-1, 5)):
    """judgment rows over docs [0, n_docs) and lists that hit them often; -> the arguments of eval_ref.eval_lists as a dict"""
    lens = rng.integers(0, max_row + 1, n_rows)
    j_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    j_doc = np.concatenate([np.sort(rng.choice(n_docs, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    j_grade = rng.integers(grades[0], grades[1] + 1, len(j_doc)).astype(np.int32)
    q_row = rng.integers(0, n_rows, nq).astype(np.int32)
    cand = np.empty((nq, m), dtype=np.int32)
    for q in range(nq):  # a permutation: no doc twice
        cand[q] = rng.permutation(n_docs)[:m] if m <= n_docs else rng.integers(0, n_docs, m)
    count = rng.integers(0, m + 1, nq).astype(np.int32)
    return dict(j_ptr=j_ptr, j_doc=j_doc, j_grade=j_grade, j_ideal=eval_ref.ideal_of(j_ptr, j_grade), cand_doc=cand, cand_count=count, q_row=q_row)


@pytest.mark.parametrize("gain,rel_level", [("linear", 1), ("exp2", 2)])
def test_fp32_restatement_against_float64(gain, rel_level):
    """The bound is DERIVED.  A table entry is one rounding of its exact value (u = 2^-24), a product one more, a sum of n
    positive terms n - 1 more: relative error (n + 1) u to first order, so |DCG32 - DCG64| <= (n + 2) u DCG64, n the positions
    the sum may take.  A ratio of two such sums (NDCG), or a sum of n rounded quotients divided once (AP): 2 (n + 3) u.  Recall, P
    and RR are ONE correctly rounded division of exact integers: u.  Integer outputs are equal."""
    rng = np.random.default_rng(7)
    nq, m, n_gain, ks = 3000, 24, 5, [1, 3, 10, 30]
    c = random_case(rng, nq, m, n_rows=400, max_row=30, n_docs=60, grades=(-1, 5))
    got = eval_ref.eval_lists(c["j_ptr"], c["j_doc"], c["j_grade"], c["j_ideal"], eval_ref.gain_table(gain, n_gain), eval_ref.discount_table(m), rel_level,
                              c["cand_doc"], c["cand_count"], c["q_row"], ks)
    assert got["n"] == nq
    sums = np.zeros((len(ks), 8))
    for q in range(nq):
        b, e = c["j_ptr"][c["q_row"][q]], c["j_ptr"][c["q_row"][q] + 1]
        judg = {int(d): int(g) for d, g in zip(c["j_doc"][b:e], c["j_grade"][b:e])}
        ranking = [int(d) for d in c["cand_doc"][q, :c["cand_count"][q]]]
        for ik, k in enumerate(ks):
            want = eval_ref.eval_query_f64(judg, ranking, k, gain, rel_level, max_grade=n_gain - 1, m=m)
            o = got["out"][q, ik].astype(np.float64)
            assert (got["hits"][q, ik], got["judged"][q, ik], got["rel"][q]) == (want["hits"], want["judged"], want["rel"])
            n = min(k, m)
            for plane, name, bound in ((eval_ref.DCG, "DCG", (n + 2) * U), (eval_ref.IDCG, "IDCG", (n + 2) * U), (eval_ref.NDCG, "NDCG", 2 * (n + 3) * U),
                                       (eval_ref.AP, "AP", 2 * (n + 3) * U), (eval_ref.RECALL, "RECALL", U), (eval_ref.P, "P", U), (eval_ref.RR, "RR", U),
                                       (eval_ref.SUCCESS, "SUCCESS", 0.0)):
                assert abs(o[plane] - want[name]) <= bound * want[name], (q, k, name, o[plane], want[name])
            sums[ik] += o
    # the means: float64 sums of the float32 values, so only the order of 3000 float64 additions separates them from this sum
    assert np.allclose(got["mean"], sums / nq, rtol=nq * 2.0 ** -53, atol=0.0)


def one_query(row: dict, ranking, ks, count=None, m=None, gain="linear", n_gain=5, rel_level=1, q_row=0):
    docs = sorted(row)
    j_ptr = np.asarray([0, len(docs)], dtype=np.int64)
    j_doc, j_grade = np.asarray(docs, dtype=np.int32), np.asarray([row[d] for d in docs], dtype=np.int32)
    m = len(ranking) if m is None else m
    cand = np.full((1, m), -1, dtype=np.int32)
    cand[0, :len(ranking)] = ranking
    return eval_ref.eval_lists(j_ptr, j_doc, j_grade, eval_ref.ideal_of(j_ptr, j_grade), eval_ref.gain_table(gain, n_gain), eval_ref.discount_table(m),
                               rel_level, cand, None if count is None else [count], [q_row], ks)


def test_cases_by_hand():
    f = np.float32
    d = eval_ref.discount_table(8)
    assert d[0] == 1.0 and d[2] == 0.5 and d[1] == f(1.0 / math.log2(3.0))
    # a perfect ranking: the list is the ideal ranking, term for term, so DCG and IDCG are the SAME float and NDCG is exactly 1
    r = one_query({1: 3, 2: 2, 5: 1, 9: 0}, [1, 2, 5, 7], [3, 4])
    for ik in (0, 1):
        o = r["out"][0, ik]
        assert o[eval_ref.NDCG] == 1.0 and o[eval_ref.AP] == 1.0 and o[eval_ref.RECALL] == 1.0 and o[eval_ref.RR] == 1.0 and o[eval_ref.SUCCESS] == 1.0
        assert o[eval_ref.DCG] == o[eval_ref.IDCG] == (f(3.0) * d[0] + f(2.0) * d[1]) + f(1.0) * d[2]
    assert r["out"][0, 0, eval_ref.P] == 1.0 and r["out"][0, 1, eval_ref.P] == f(3.0) / f(4.0)
    assert r["hits"].tolist() == [[3, 3]] and r["judged"].tolist() == [[3, 3]] and r["rel"].tolist() == [3] and r["n"] == 1
    # one relevant doc at rank 3, another one never retrieved: R = 2
    r = one_query({7: 1, 9: 1, 4: 0}, [3, 4, 7, 8], [2, 3, 4])
    o = r["out"][0]
    assert not o[0, :eval_ref.IDCG].any() and o[0, eval_ref.IDCG] == f(1.0) * d[0] + f(1.0) * d[1] and r["hits"][0].tolist() == [0, 1, 1] and r["judged"][0].tolist() == [1, 2, 2]
    idcg = f(1.0) * d[0] + f(1.0) * d[1]
    for ik in (1, 2):
        assert o[ik, eval_ref.RR] == f(1.0) / f(3.0) and o[ik, eval_ref.AP] == (f(1.0) / f(3.0)) / f(2.0)
        assert o[ik, eval_ref.DCG] == 0.5 and o[ik, eval_ref.IDCG] == idcg and o[ik, eval_ref.NDCG] == f(0.5) / idcg
        assert o[ik, eval_ref.RECALL] == 0.5 and o[ik, eval_ref.SUCCESS] == 1.0
    assert o[1, eval_ref.P] == f(1.0) / f(3.0) and o[2, eval_ref.P] == 0.25
    # k greater than the list: n = 2 positions, P still divides by k, IDCG takes min(k, row, m) = 2 of the 3 judged
    r = one_query({1: 1, 2: 1, 3: 1}, [2, 9, 1, 3], [10], count=2)
    o = r["out"][0, 0]
    assert r["hits"].tolist() == [[1]] and o[eval_ref.P] == f(1.0) / f(10.0) and o[eval_ref.RECALL] == f(1.0) / f(3.0)
    assert o[eval_ref.AP] == f(1.0) / f(3.0) and o[eval_ref.DCG] == 1.0 and o[eval_ref.IDCG] == (d[0] + d[1]) + d[2]
    r = one_query({1: 1, 2: 1, 3: 1}, [2, 9], [10])  # the same list stored at m = 2: the ideal ranking is cut at m
    assert r["out"][0, 0, eval_ref.IDCG] == d[0] + d[1]
    # R = 0: judged, nothing relevant (a negative grade is judged, and non-relevant) -- evaluated, all zeros
    r = one_query({1: 0, 2: -3}, [1, 2, 3], [3])
    assert not r["out"].any() and r["hits"].tolist() == [[0]] and r["judged"].tolist() == [[2]] and r["rel"].tolist() == [0] and r["n"] == 1
    assert not r["mean"].any()
    # a query that is not judged: zeros, and left out of the means
    for row in (-1, 1, 99):
        r = one_query({1: 3}, [1], [1], q_row=row)
        assert not r["out"].any() and r["hits"].tolist() == [[0]] and r["judged"].tolist() == [[0]] and r["rel"].tolist() == [0]
        assert r["n"] == 0 and not r["mean"].any() and not np.signbit(r["mean"]).any()
    # a grade above the table clamps; rel_level 2; exp2 gains; a doc twice counts twice
    r = one_query({1: 9, 2: 1}, [2, 1, 1], [3], gain="exp2", n_gain=3, rel_level=2)
    o = r["out"][0, 0]
    assert r["hits"].tolist() == [[2]] and r["rel"].tolist() == [1] and o[eval_ref.RECALL] == 2.0
    assert o[eval_ref.DCG] == (f(1.0) * d[0] + f(3.0) * d[1]) + f(3.0) * d[2] and o[eval_ref.IDCG] == f(3.0) * d[0] + f(1.0) * d[1]
    assert o[eval_ref.AP] == (f(1.0) / f(2.0) + f(2.0) / f(3.0)) / f(1.0) and o[eval_ref.RR] == 0.5


def test_means_by_chunks():
    """1 025 evaluated queries: chunk 0 holds 1 024 of them, chunk 1 the last; an unjudged query in between adds nothing"""
    rng = np.random.default_rng(3)
    c = random_case(rng, 1030, 5, n_rows=50, max_row=6, n_docs=12, grades=(0, 3))
    c["q_row"][[5, 100, 1024, 1026, 1029]] = [-1, 50, -1, 77, -1]
    r = eval_ref.eval_lists(c["j_ptr"], c["j_doc"], c["j_grade"], c["j_ideal"], eval_ref.gain_table("linear", 4), eval_ref.discount_table(5), 1,
                            c["cand_doc"], c["cand_count"], c["q_row"], [1, 5])
    assert r["n"] == 1025
    vals = r["out"].astype(np.float64)
    first = np.zeros((2, 8))
    for q in range(1024):
        first = first + vals[q]
    second = np.zeros((2, 8))
    for q in range(1024, 1030):
        second = second + vals[q]
    assert np.array_equal(r["mean"], (first + second) / 1025.0)


# ---- Judgments ----------------------------------------------------------------------------------------------------------------------
CORPUS = ["d0", "d1", "d2", "d3", "d4", "d5"]
QRELS = {"q1": {"d3": 2, "d0": 1, "gone": 3, "d5": 0}, "q2": {"d1": 1}, "q3": {}, "q4": {"lost": 1, "gone": -1}}


def test_from_qrels():
    j = ev.Judgments.from_qrels(QRELS, None, CORPUS)
    assert (j.n_rows, j.nnz, j.query_ids, j.device) == (4, 7, ["q1", "q2", "q3", "q4"], None)
    assert j.j_ptr.dtype == np.int64 and j.j_ptr.tolist() == [0, 4, 5, 5, 7]
    # rows sorted by doc; a judged doc that is not in the corpus gets an id past it, in the order of first appearance
    assert j.extra_ids == {"gone": 6, "lost": 7}
    assert j.j_doc.dtype == np.int32 and j.j_doc.tolist() == [0, 3, 5, 6, 1, 6, 7]
    assert j.j_grade.tolist() == [1, 2, 0, 3, 1, -1, 1] and j.j_ideal.tolist() == [3, 2, 1, 0, 1, 1, -1]
    for r in range(j.n_rows):
        b, e = j.j_ptr[r], j.j_ptr[r + 1]
        assert (np.diff(j.j_doc[b:e]) > 0).all() and (np.diff(j.j_ideal[b:e]) <= 0).all()
        assert sorted(j.j_ideal[b:e].tolist()) == sorted(j.j_grade[b:e].tolist())
    assert np.array_equal(j.j_ideal, eval_ref.ideal_of(j.j_ptr, j.j_grade))
    assert (j.max_grade, j.n_gain) == (3, 4)
    # the doc outside the corpus raises R and the ideal ranking: it can never be retrieved, recall stays below 1
    qids, doc, count, q_rows = ev.lists_from_results(j, {"q1": {"d3": 2.0, "d0": 1.0}})
    r = eval_ref.eval_lists(j.j_ptr, j.j_doc, j.j_grade, j.j_ideal, eval_ref.gain_table("linear", 4), eval_ref.discount_table(2), 1, doc, count, q_rows, [10])
    assert r["rel"].tolist() == [3] and r["out"][0, 0, eval_ref.RECALL] == np.float32(2.0) / np.float32(3.0) and r["out"][0, 0, eval_ref.NDCG] < 1.0
    # query_ids picks and orders the rows; an id without judgments is an empty row; an entry outside is left out
    j = ev.Judgments.from_qrels(QRELS, ["q2", "zz", "q1"], CORPUS)
    assert j.j_ptr.tolist() == [0, 1, 1, 5] and j.row_of == {"q2": 0, "zz": 1, "q1": 2} and j.extra_ids == {"gone": 6}
    # an empty qrels
    j = ev.Judgments.from_qrels({}, None, CORPUS)
    assert (j.n_rows, j.nnz, j.j_ptr.tolist(), j.n_gain) == (0, 0, [0], 2)
    with pytest.raises(ValueError, match="twice"):
        ev.Judgments.from_qrels({"q1": [("d1", 1), ("d2", 0), ("d1", 2)]}, None, CORPUS)
    with pytest.raises(ValueError, match="twice"):
        ev.Judgments.from_qrels(QRELS, ["q1", "q1"], CORPUS)
    for bad in (1.0, "1", None, True):
        with pytest.raises(ValueError, match="a grade must be an int"):
            ev.Judgments.from_qrels({"q1": {"d1": bad}}, None, CORPUS)
    with pytest.raises(ValueError, match="without a device"):
        ev.Judgments.from_qrels(QRELS, None, CORPUS).evaluate(np.zeros((1, 1), np.int32))


def test_from_arrays():
    j = ev.Judgments.from_arrays([2, 0, 2, 0], [9, 5, 3, 1], [1, 0, 4, 2], n_rows=4)
    assert j.j_ptr.tolist() == [0, 2, 2, 4, 4] and j.j_doc.tolist() == [1, 5, 3, 9] and j.j_grade.tolist() == [2, 0, 4, 1] and j.j_ideal.tolist() == [2, 0, 4, 1]
    assert ev.Judgments.from_arrays([1], [7], [40]).n_gain == 32 and ev.Judgments.from_arrays([], [], []).n_rows == 0
    for args, word in ((([0, 0], [3, 3], [1, 2]), "twice"), (([0], [1, 2], [1, 1]), "one length"), (([0.5], [1], [1]), "integer"),
                       (([3], [1], [1], 3), "row must be in"), (([-1], [1], [1]), "row must be in"), (([0], [2 ** 31], [1]), "doc id must fit int32"),
                       (([0], [1], [-2 ** 31 - 1]), "grade must fit int32")):
        with pytest.raises(ValueError, match=word):
            ev.Judgments.from_arrays(*args)


def test_tables_and_cutoffs():
    assert ev.gain_table("linear", 5).tolist() == [0, 1, 2, 3, 4] and ev.gain_table("exp2", 5).tolist() == [0, 1, 3, 7, 15]
    assert ev.gain_table("exp2", 32)[31] == np.float32(2.0 ** 31 - 1) and ev.gain_table("exp2", 1).tolist() == [0.0] and not np.signbit(ev.gain_table("exp2", 1)[0])
    for kind in ev.GAINS:
        assert np.array_equal(ev.gain_table(kind, 32), eval_ref.gain_table(kind, 32))
    assert np.array_equal(ev.discount_table(2048), eval_ref.discount_table(2048)) and ev.discount_table(2048).dtype == np.float32
    assert ev.check_cutoffs((1, 3, 5, 10, 100)) == [1, 3, 5, 10, 100] and ev.check_cutoffs([2048], cap=2048) == [2048]
    for ks in ((), (0,), (3, 3), (5, 1), tuple(range(1, 10)), (1.5,), 7):
        with pytest.raises(ValueError, match="k_values"):
            ev.check_cutoffs(ks)
    with pytest.raises(ValueError, match="cutoff above 2048"):
        ev.check_cutoffs((1, 2049), cap=2048)
    with pytest.raises(ValueError, match="gain must be"):
        ev.gain_table("log", 4)
    with pytest.raises(ValueError, match="n_gain"):
        ev.gain_table("linear", 33)


# ---- the dict door --------------------------------------------------------------------------------------------------------------------
def door(qrels, results, k_values, corpus=CORPUS, gain="linear", rel_level=1, per_query=False, complete=False, ignore_identical_ids=False):
    """evaluate.evaluate_results with the restatement in the place of the device call"""
    ks = ev.check_cutoffs(k_values, cap=2048)
    j = ev.Judgments.from_qrels(qrels, None, corpus)
    qids, doc, count, q_rows = ev.lists_from_results(j, results, complete, ignore_identical_ids)
    r = eval_ref.eval_lists(j.j_ptr, j.j_doc, j.j_grade, j.j_ideal, ev.gain_table(gain, j.n_gain), ev.discount_table(doc.shape[1]), rel_level, doc, count,
                            q_rows, ks)
    res = ev.EvalResult(r["out"], r["hits"], r["judged"], r["rel"], r["mean"], r["n"])
    return ev.metrics_dicts(res, ks, qids if per_query else None)


def test_dict_door():
    results = {"q1": {"d0": 3.0, "d3": 5.0, "d2": 4.0}, "q2": {"d4": 1.0, "d1": 0.5}, "q9": {"d1": 1.0}}
    agg, per = door(QRELS, results, (1, 3), per_query=True)
    assert list(agg) == ["NDCG@1", "MAP@1", "Recall@1", "P@1", "MRR@1", "Success@1", "Judged@1", "NDCG@3", "MAP@3", "Recall@3", "P@3", "MRR@3", "Success@3",
                         "Judged@3", "n_queries"]
    assert agg["n_queries"] == 2 and set(per) == {"q1", "q2"} and list(per["q1"]) == list(agg)[:-1]  # q9 is not judged, q3 / q4 have no results
    assert all(isinstance(v, float) for v in per["q1"].values()) and isinstance(agg["n_queries"], int)
    # q1 ranks d3 (2), d2 (unjudged), d0 (1); R = 3 with the doc outside the corpus
    want = eval_ref.eval_query_f64({"d3": 2, "d0": 1, "gone": 3, "d5": 0}, ["d3", "d2", "d0"], 3, max_grade=3)
    for key, name in (("NDCG@3", "NDCG"), ("MAP@3", "AP"), ("Recall@3", "RECALL"), ("P@3", "P"), ("MRR@3", "RR"), ("Success@3", "SUCCESS")):
        assert per["q1"][key] == pytest.approx(want[name], rel=1e-6), key
    assert per["q1"]["Judged@3"] == 2 / 3 and per["q1"]["Judged@1"] == 1.0 and per["q2"]["Judged@3"] == 1 / 3 and per["q2"]["MRR@3"] == 0.5
    for key in agg:
        if key != "n_queries":
            assert agg[key] == pytest.approx((per["q1"][key] + per["q2"][key]) / 2, rel=1e-12), key
    assert door(QRELS, results, (1, 3)) == agg
    # complete: every judged query is evaluated; one without results scores zeros
    full, per_full = door(QRELS, results, (3,), per_query=True, complete=True)
    assert full["n_queries"] == 4 and list(per_full) == ["q1", "q2", "q3", "q4"] and not any(per_full["q3"].values()) and not any(per_full["q4"].values())
    assert full["NDCG@3"] == pytest.approx(agg["NDCG@3"] / 2, rel=1e-12)
    # the order rule: score descending, then corpus order, whatever the dict's order; a doc outside the corpus behind it; NaN last
    j = ev.Judgments.from_qrels(QRELS, None, CORPUS)
    _, doc, count, _ = ev.lists_from_results(j, {"q1": {"zz": 2.0, "d4": 2.0, "gone": 2.0, "d1": 2.0, "d5": float("nan"), "d2": 7.0, "d0": float("-inf")}})
    assert doc.tolist() == [[2, 1, 4, 6, -1, 0, 5]] and count.tolist() == [7]
    # ignore_identical_ids drops doc_id == qid before the ranking
    corpus = CORPUS + ["q1"]
    res = {"q1": {"q1": 9.0, "d3": 1.0}}
    plain, dropped = door(QRELS, res, (1,), corpus=corpus), door(QRELS, res, (1,), corpus=corpus, ignore_identical_ids=True)
    assert (plain["Success@1"], dropped["Success@1"]) == (0.0, 1.0)
    # lists deeper than 2 048 are cut there; no list at all
    deep = {"q2": {f"x{i}": float(-i) for i in range(3000)}}
    _, doc, count, _ = ev.lists_from_results(j, deep)
    assert doc.shape == (1, 2048) and count.tolist() == [2048]
    _, doc, count, q_rows = ev.lists_from_results(j, {})
    assert doc.shape == (0, 1) and len(count) == len(q_rows) == 0 and door(QRELS, {}, (1,))["n_queries"] == 0
    with pytest.raises(ValueError, match="cutoff above 2048"):
        door(QRELS, results, (10, 4096))
    with pytest.raises(ValueError, match="from_qrels"):
        ev.lists_from_results(ev.Judgments.from_arrays([0], [1], [1]), results)


def test_doors_and_signatures():
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(SparseIndexViews.evaluate) == ["self", "qrels", "results", "k_values", "gain", "rel_level", "per_query", "complete", "ignore_identical_ids"]
    sig = inspect.signature(SparseIndexViews.evaluate)
    assert sig.parameters["k_values"].default == (1, 3, 5, 10, 100) == ev.DEFAULT_K_VALUES
    assert [p.kind for p in sig.parameters.values()][4:] == [inspect.Parameter.KEYWORD_ONLY] * 5
    assert [sig.parameters[n].default for n in names(SparseIndexViews.evaluate)[4:]] == ["linear", 1, False, False, False]
    assert names(SparseIndexViews.rank_eval) == ["self", "queries", "qrels", "k_values", "search_keywords"]
    assert names(ev.evaluate_results)[:5] == ["qrels", "results", "doc_ids", "device", "k_values"] and names(ev.evaluate_results)[5:] == names(SparseIndexViews.evaluate)[4:]
    assert names(ev.Judgments.evaluate_device) == ["self", "doc", "count", "ks", "q_rows", "gain", "rel_level", "means", "n_gain"]
    assert names(ev.Judgments.evaluate) == ["self", "doc", "count", "ks", "q_rows", "gain", "rel_level", "means", "n_gain"]
    assert names(ev.Judgments.from_qrels) == ["qrels", "query_ids", "doc_ids", "device"]
    for cls, door_name in ((sparse_rx.RetrievalService, "search_bm25"), (sparse_rx.OptimizedBM25Retriever, "search"), (sparse_rx.OptimizedRetriever, "search")):
        assert cls.evaluate is SparseIndexViews.evaluate and cls.rank_eval is SparseIndexViews.rank_eval
        assert cls.search_door == door_name and callable(getattr(cls, door_name))
    for cls in (sparse_rx.HybridRetriever, sparse_rx.HostBatchPipeline):
        assert not hasattr(cls, "evaluate") and not hasattr(cls, "rank_eval")
    # the searches took no new keyword
    for f in (sparse_rx.RetrievalService.search_bm25, sparse_rx.OptimizedBM25Retriever.search, sparse_rx.RetrievalService.search_hybrid):
        assert not {"qrels", "k_values", "evaluate"} & set(names(f))
    # before an index is built the doors say so, and rank_eval checks its cutoffs before it searches
    svc = sparse_rx.RetrievalService.__new__(sparse_rx.RetrievalService)
    svc._be = type("NoIndex", (), {"host": None, "dev": None})()
    with pytest.raises(ValueError, match="not built"):
        svc.evaluate(QRELS, {})
    with pytest.raises(ValueError, match="k_values"):
        svc.rank_eval({"q1": "text"}, QRELS, (3, 1))
    with pytest.raises(ValueError, match="give no top_k"):
        svc.rank_eval({"q1": "text"}, QRELS, (1, 3), top_k=5)
