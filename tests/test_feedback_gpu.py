"""Relevance feedback on the GPU (include/ext/sparse_rx_feedback.h).  Expected rows are never the engine's own: the restatement
(tests/feedback_ref.py) for the expansion, ``oracle.search_batch`` for the searches.  Every comparison is exact -- term ids,
row pointers and the BITS of the weights --, and every output buffer is pre-filled with 0x7f bytes so that a word the kernels
do not write, or write and should not, shows."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import feedback_ref  # noqa: E402
from feedback_ref import BY_SCORE, RAW, RM, UNIFORM  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda:0"
GARBAGE = 0x7F7F7F7F
N_DOCS, VOCAB, PER_DOC, BASE, NQ, M = 3000, 500, 20, 1000, 33, 40
I32_MAX, I32_MIN = 2 ** 31 - 1, -(2 ** 31)


class _Forward:
    """A forward index on the device as the C call takes it -- the rows are the restatement's, not ForwardIndex's -- next to its
    host arrays"""

    def __init__(self, corpus, idf, doc_base=BASE):
        import torch
        from sparse_rx import _capi
        self.row_ptr, self.term, self.value, self.longest = feedback_ref.forward_rows(corpus.indptr, corpus.indices, corpus.data, idf)
        self.doc_len = np.ascontiguousarray(corpus.doc_lengths, dtype=np.float32)
        self.n_docs, self.vocab, self.doc_base = len(self.row_ptr) - 1, int(corpus.vocab), doc_base
        self.t = [torch.from_numpy(x).to(DEVICE) for x in (self.row_ptr, self.term, self.value, self.doc_len)]
        self.desc = _capi.ForwardDesc(device=0, reserved=0, n_docs=self.n_docs, vocab=self.vocab, doc_base=doc_base, row_ptr=self.t[0].data_ptr(),
                                      term=self.t[1].data_ptr(), value=self.t[2].data_ptr(), doc_len=self.t[3].data_ptr())

    def run(self, batch, fb, fb_docs, n_terms=10, row_cap=None, doc_weight=BY_SCORE, term_weight=RM, alpha=0.5, beta=0.5, gain=None, stream=None,
            outs=None):
        """The C call on fresh (or the given) garbage-filled outputs -> host (out_ptr, out_term, out_weight, flag) with the whole
        buffers, and the device outputs"""
        import torch
        from sparse_rx import _capi
        q_ptr, q_term, q_weight = batch
        fb_doc, fb_score, fb_count = fb
        nq, m = len(q_ptr) - 1, fb_doc.shape[1]
        up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(DEVICE)
        ins = [up(q_ptr, np.int32), up(q_term, np.int32), up(q_weight, np.float32), up(fb_doc, np.int32), up(fb_score, np.float32), up(fb_count, np.int32),
               up(gain, np.float32)]
        row_cap = max(1, min(self.longest, 4096 // fb_docs)) if row_cap is None else row_cap
        par = _capi.FeedbackParams(fb_docs=fb_docs, row_cap=row_cap, n_terms=n_terms, doc_weight=doc_weight, term_weight=term_weight, alpha=alpha, beta=beta)
        cap = len(q_term) + nq * n_terms
        L = _capi.lib()
        if outs is None:
            outs = [torch.full((n,), GARBAGE, dtype=torch.int32, device=DEVICE) for n in (nq + 1, cap + 5, cap + 5, 1)]
        ws = torch.full((int(L.srx_feedback_workspace_bytes(nq)) // 4,), GARBAGE, dtype=torch.int32, device=DEVICE)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        torch.cuda.synchronize()
        sp = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
        rc = L.srx_feedback_expand(ctypes.byref(self.desc), ctypes.byref(par), ptr(ins[6]), ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), nq, len(q_term),
                                   ptr(ins[3]), ptr(ins[4]), ptr(ins[5]), m, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), cap, ptr(outs[3]), ptr(ws),
                                   ws.numel() * 4, sp)
        _capi.check(rc, "srx_feedback_expand")
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs], outs

    def expect(self, batch, fb, fb_docs, n_terms=10, row_cap=None, doc_weight=BY_SCORE, term_weight=RM, alpha=0.5, beta=0.5, gain=None):
        row_cap = max(1, min(self.longest, 4096 // fb_docs)) if row_cap is None else row_cap
        return feedback_ref.expand(self.row_ptr, self.term, self.value, self.doc_len, self.n_docs, self.doc_base, fb_docs, row_cap, n_terms, doc_weight,
                                   term_weight, alpha, beta, gain, *batch, *fb)

    def check(self, batch, fb, fb_docs, label="", **kw):
        run_kw = {k: kw.pop(k) for k in ("stream", "outs") if k in kw}
        got, outs = self.run(batch, fb, fb_docs, **kw, **run_kw)
        e_ptr, e_term, e_weight, e_flag = self.expect(batch, fb, fb_docs, **kw)
        n = int(e_ptr[-1])
        assert np.array_equal(got[0], e_ptr), (label, "out_ptr", got[0], e_ptr)
        assert np.array_equal(got[1][:n], e_term), (label, "out_term")
        assert np.array_equal(got[2][:n], e_weight.view(np.int32)), (label, "out_weight")
        assert (got[1][n:] == GARBAGE).all() and (got[2][n:] == GARBAGE).all(), (label, "written at or behind out_ptr[nq]")
        assert int(got[3][0]) == e_flag, (label, "flag")
        return (e_ptr, e_term, e_weight, e_flag), outs


@pytest.fixture(scope="module")
def world():
    """The corpus, its forward index, 33 queries of 4 terms and the oracle's own first pass, 40 deep (global ids)"""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import oracle
    import sparse_rx
    from sparse_rx import synth
    sparse_rx._capi.lib()
    c = synth.uniform_corpus_np(N_DOCS, VOCAB, PER_DOC, seed=11)
    _, idf, avgdl = synth.corpus_stats(c)
    batch = synth.queries_np(NQ, VOCAB, 4, seed=12)
    d, s, n = oracle.search_batch(c.indptr, c.indices, c.data, c.doc_lengths, idf, *batch, M, 1.2, 0.75, avgdl)
    fb = (np.where(d >= 0, d + BASE, d).astype(np.int32), s.astype(np.float32), n.astype(np.int32))
    return {"corpus": c, "idf": idf, "avgdl": avgdl, "fwd": _Forward(c, idf), "batch": batch, "fb": fb}


def test_forward_index_rows_are_the_restatement(world):
    from sparse_rx import ForwardIndex
    c, f = world["corpus"], world["fwd"]
    ix = ForwardIndex.from_csr(c.indptr, c.indices, c.data, world["idf"], doc_lengths=c.doc_lengths, device=DEVICE, doc_base=BASE)
    assert np.array_equal(ix.row_ptr.cpu().numpy(), f.row_ptr) and np.array_equal(ix.term.cpu().numpy(), f.term)
    assert np.array_equal(ix.value.cpu().numpy().view(np.int32), f.value.view(np.int32)) and ix.max_row_terms == f.longest
    assert ix.device_bytes() == 8 * len(f.term) + 8 * (N_DOCS + 1) + 4 * N_DOCS and (ix.n_docs, ix.vocab, ix.doc_base) == (N_DOCS, VOCAB, BASE)
    # the door on host arrays gives the restatement's batch
    got = ix.expand(*world["batch"], *world["fb"], fb_docs=10, n_terms=10, term_gain=np.maximum(world["idf"], 0))
    exp = f.expect(world["batch"], world["fb"], 10, gain=np.maximum(world["idf"], 0))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and np.array_equal(got[2].view(np.int32), exp[2].view(np.int32)) and got[3] == 0
    ix.close()
    with pytest.raises(ValueError, match="closed"):
        ix.expand(*world["batch"], *world["fb"], fb_docs=10)


@pytest.mark.parametrize("fb_docs", [1, 10, 32])
def test_feedback_depths(world, fb_docs):
    exp, _ = world["fwd"].check(world["batch"], world["fb"], fb_docs, label=f"R={fb_docs}")
    extra = np.diff(exp[0]) - np.diff(world["batch"][0])
    assert extra.min() >= 0 and extra.max() <= 10 and extra.sum() > 0  # the query's terms and up to 10 more
    if fb_docs == 10:  # the A + B path: nearly every query term is also selected
        e_ptr, e_term, _, _ = world["fwd"].expect(world["batch"], world["fb"], 10, alpha=0.0, beta=1.0)
        q_ptr, q_term, _ = world["batch"]
        both = sum(len(set(q_term[q_ptr[q]: q_ptr[q + 1]]) & set(e_term[e_ptr[q]: e_ptr[q + 1]])) for q in range(NQ))
        assert both > len(q_term) // 2


@pytest.mark.parametrize("row_cap", [1, 7, "row", 64])
def test_row_caps(world, row_cap):
    f = world["fwd"]
    cap = f.longest if row_cap == "row" else row_cap
    assert f.longest < 64
    f.check(world["batch"], world["fb"], 10, row_cap=cap, label=f"row_cap={cap}")


def test_full_budget():
    """400 docs with rows of exactly 128 terms, R = 32, row_cap = 128: 4 096 pairs per query, 128 expansion terms"""
    from sparse_rx import synth
    rng = np.random.default_rng(5)
    n, vocab = 400, 1500
    terms = np.stack([np.sort(rng.choice(vocab, 128, replace=False)) for _ in range(n)]).astype(np.int32)
    tf = rng.integers(1, 6, terms.shape).astype(np.float32)
    c = synth.CsrCorpus(np.arange(0, 128 * n + 1, 128, dtype=np.int64), terms.reshape(-1), tf.reshape(-1), tf.sum(axis=1).astype(np.float32), vocab)
    _, idf, _ = synth.corpus_stats(c)
    f = _Forward(c, idf, doc_base=0)
    assert f.longest == 128
    batch = synth.queries_np(5, vocab, 6, seed=3)
    fb_doc = np.stack([rng.choice(n, 32, replace=False) for _ in range(5)]).astype(np.int32)
    fb_score = np.sort(rng.random((5, 32)).astype(np.float32) + 0.1, axis=1)[:, ::-1]
    for n_terms, dw in ((128, BY_SCORE), (10, UNIFORM)):
        exp, _ = f.check(batch, (fb_doc, fb_score, None), 32, n_terms=n_terms, row_cap=128, doc_weight=dw, gain=np.maximum(idf, 0), label=f"full n_terms={n_terms}")
    assert np.diff(exp[0]).max() <= 16


@pytest.mark.parametrize("n_terms", [1, 128])
def test_term_counts(world, n_terms):
    exp, _ = world["fwd"].check(world["batch"], world["fb"], 10, n_terms=n_terms, label=f"n_terms={n_terms}")
    if n_terms == 128:  # the candidates of 10 rows of <= 20 terms: every query selects 128
        assert np.diff(exp[0]).min() >= 128
    # more than there are candidates: 2 docs of <= 20 terms hold fewer than 128
    exp, _ = world["fwd"].check(world["batch"], world["fb"], 2, n_terms=128, label="more than candidates")
    assert np.diff(exp[0]).max() < 60


@pytest.mark.parametrize("doc_weight", [BY_SCORE, UNIFORM])
@pytest.mark.parametrize("term_weight", [RM, RAW])
def test_modes(world, doc_weight, term_weight):
    f = world["fwd"]
    f.check(world["batch"], world["fb"], 10, doc_weight=doc_weight, term_weight=term_weight, gain=np.maximum(world["idf"], 0), label="modes")
    if doc_weight == UNIFORM:  # the scores are not looked at
        d, s, n = world["fb"]
        got, _ = f.run(world["batch"], (d, None, n), 10, doc_weight=UNIFORM, term_weight=term_weight)
        e = f.expect(world["batch"], (d, s, n), 10, doc_weight=UNIFORM, term_weight=term_weight)
        assert np.array_equal(got[0], e[0]) and np.array_equal(got[2][: int(e[0][-1])], e[2].view(np.int32))


def test_gains(world):
    f, batch, fb, idf = world["fwd"], world["batch"], world["fb"], world["idf"]
    f.check(batch, fb, 10, gain=None, label="gain NULL")
    f.check(batch, fb, 10, gain=idf, label="gain idf")
    # all zero: no candidate, the row is the normalised query
    exp, _ = f.check(batch, fb, 10, gain=np.zeros(VOCAB, np.float32), label="gain 0")
    q_ptr, q_term, q_weight = batch
    assert np.array_equal(exp[0], q_ptr) and np.array_equal(exp[1], q_term)
    for q in range(NQ):
        w = q_weight[q_ptr[q]: q_ptr[q + 1]]
        total = np.float32(0)
        for x in w:
            total = np.float32(total + x)
        assert np.array_equal(exp[2][q_ptr[q]: q_ptr[q + 1]], np.float32(0.5) * (w / total))
    # one banned term that would otherwise win: the best expansion term of query 0 under gain 1
    e_ptr, e_term, e_weight, _ = f.expect(batch, fb, 10, n_terms=1, alpha=0.0, beta=1.0)
    winner = int(e_term[e_ptr[0]])
    gain = np.ones(VOCAB, np.float32)
    gain[winner] = 0
    exp, _ = f.check(batch, fb, 10, n_terms=1, alpha=0.0, beta=1.0, gain=gain, label="banned")
    assert int(exp[0][1]) == 1 and int(exp[1][0]) != winner
    gain[winner] = -1  # a negative gain bans as well
    f.check(batch, fb, 10, gain=gain, label="negative gain")


def test_counts_docs_and_scores(world):
    f, batch = world["fwd"], world["batch"]
    d, s, n = (x.copy() for x in world["fb"])
    # fb_count: 0, negative, above m, NULL
    n[0], n[1], n[2], n[3] = 0, -5, M + 9, I32_MIN
    f.check(batch, (d, s, n), 10, label="counts")
    f.check(batch, (d, s, n), 32, label="counts R=32")
    f.check(batch, (d, s, None), 10, label="count NULL")
    # docs: -1, below doc_base, past the end, a doc listed twice; all of a list outside
    d[4, 0], d[4, 1], d[4, 2], d[4, 3] = -1, BASE - 1, BASE + N_DOCS, d[4, 4]
    d[5, :3] = d[5, 3]
    d[6, :] = [-1, 0, BASE - 1, BASE + N_DOCS, I32_MAX, I32_MIN] * 6 + [-1] * 4
    exp, _ = f.check(batch, (d, s, None), 10, label="docs")
    assert exp[0][7] - exp[0][6] == batch[0][7] - batch[0][6]  # no used doc: the normalised query
    f.check(batch, (d, s, None), 10, doc_weight=UNIFORM, label="docs uniform")
    # scores: 0, negative, NaN and +inf are not used under BY_SCORE; -0 and -inf neither
    s[8, :6] = [0.0, -1.0, np.nan, np.inf, -0.0, -np.inf]
    s[9, :] = np.nan
    s[10, 0] = np.float32(1e-42)  # a denormal score is positive
    f.check(batch, (d, s, None), 10, label="scores")
    f.check(batch, (d, s, None), 10, doc_weight=UNIFORM, label="scores uniform")  # ... and all of them are under UNIFORM


def test_empty_and_absent(world):
    f = world["fwd"]
    q_ptr, q_term, q_weight = world["batch"]
    d, s, n = (x.copy() for x in world["fb"])
    # query 1 loses its terms; query 2 loses them and every used doc: an empty row, out_ptr repeats; the last query is empty too
    keep = np.ones(len(q_term), bool)
    keep[q_ptr[1]: q_ptr[3]] = False
    keep[q_ptr[NQ - 1]:] = False
    lens = np.diff(q_ptr)
    lens[[1, 2, NQ - 1]] = 0
    p2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n[2] = 0
    d[NQ - 1, :] = -1
    exp, _ = f.check((p2, q_term[keep], q_weight[keep]), (d, s, n), 10, label="empty queries")
    assert exp[0][2] - exp[0][1] == 10 and exp[0][3] == exp[0][2] and exp[0][NQ] == exp[0][NQ - 1]
    # a query term that appears in no feedback doc: a term no doc of the corpus holds
    c = world["corpus"]
    absent = int(np.setdiff1d(np.arange(VOCAB), c.indices[c.indptr[int(d[0, 0]) - BASE]: c.indptr[int(d[0, 0]) - BASE + 1]])[0])
    t2 = q_term.copy()
    t2[0] = absent
    t2[: q_ptr[1]] = np.sort(t2[: q_ptr[1]])
    assert len(set(t2[: q_ptr[1]])) == q_ptr[1]
    exp, _ = f.check((q_ptr, t2, q_weight), (d, s, n), 1, label="absent term")
    assert absent in exp[1][: exp[0][1]]
    # alpha = 0: query terms that are not selected vanish; beta = 0: the normalised query at alpha
    exp, _ = f.check(world["batch"], world["fb"], 10, n_terms=2, alpha=0.0, beta=1.0, label="alpha 0")
    assert (np.diff(exp[0]) == 2).all()
    exp, _ = f.check(world["batch"], world["fb"], 10, alpha=0.75, beta=0.0, label="beta 0")
    assert np.array_equal(exp[0], q_ptr) and np.array_equal(exp[1], q_term)
    f.check(world["batch"], world["fb"], 10, alpha=3.0, beta=0.25, label="weights above 1")


def test_over_long_query_passes_through(world):
    f = world["fwd"]
    q_ptr, q_term, q_weight = world["batch"]
    rng = np.random.default_rng(9)
    long_terms = rng.choice(VOCAB, 129, replace=False).astype(np.int32)  # not sorted: the order is kept
    long_w = rng.random(129).astype(np.float32)
    rows = [(q_term[q_ptr[q]: q_ptr[q + 1]], q_weight[q_ptr[q]: q_ptr[q + 1]]) for q in range(NQ)]
    rows[5] = (long_terms, long_w)
    p2 = np.concatenate([[0], np.cumsum([len(t) for t, _ in rows])]).astype(np.int32)
    t2, w2 = np.concatenate([t for t, _ in rows]), np.concatenate([w for _, w in rows])
    exp, _ = f.check((p2, t2, w2), world["fb"], 10, label="129 terms")
    assert exp[3] == 1 and np.array_equal(exp[1][exp[0][5]: exp[0][6]], long_terms) and np.array_equal(exp[2][exp[0][5]: exp[0][6]], long_w)
    plain, _ = f.check(world["batch"], world["fb"], 10, label="neighbours")
    for q in (4, 6, NQ - 1):  # the neighbours' rows are what they are without it
        assert np.array_equal(exp[1][exp[0][q]: exp[0][q + 1]], plain[1][plain[0][q]: plain[0][q + 1]])
        assert np.array_equal(exp[2][exp[0][q]: exp[0][q + 1]].view(np.int32), plain[2][plain[0][q]: plain[0][q + 1]].view(np.int32))
    # exactly 128 terms is expanded
    p3 = np.array([0, 128], dtype=np.int32)
    t3 = np.sort(long_terms[:128])
    exp, _ = f.check((p3, t3, long_w[:128]), tuple(x[:1] for x in world["fb"]), 10, n_terms=128, label="128 terms")
    assert exp[3] == 0 and exp[0][1] > 128


def test_ties_in_the_selection_key(world):
    """tf = 1 everywhere, uniform doc weights, raw values: fb(t) = (docs that hold t) / 10 -- a handful of distinct values over
    about 150 candidates, so every cut falls inside a tie and goes to the smaller term ids"""
    from sparse_rx import synth
    c = world["corpus"]
    ones = synth.CsrCorpus(c.indptr, c.indices, np.ones_like(c.data), np.diff(c.indptr).astype(np.float32), c.vocab)
    f = _Forward(ones, np.ones(VOCAB, np.float32))
    for n_terms in (7, 10, 64):
        exp, _ = f.check(world["batch"], world["fb"], 10, n_terms=n_terms, doc_weight=UNIFORM, term_weight=RAW, alpha=0.0, beta=1.0, label="ties")
        rows = [exp[2][exp[0][q]: exp[0][q + 1]] for q in range(NQ)]
        assert all(len(r) == n_terms for r in rows) and sum(len(set(r.tolist())) < len(r) for r in rows) > NQ // 2


def test_stream_and_rerun(world):
    import torch
    f = world["fwd"]
    stream = torch.cuda.Stream(device=DEVICE)
    with torch.cuda.stream(stream):
        f.check(world["batch"], world["fb"], 10, stream=stream, label="stream")
    # two runs into the same buffers give the same bytes (the second over the first's output, not over garbage)
    exp, outs = f.check(world["batch"], world["fb"], 10, label="first")
    first = [o.cpu().numpy().copy() for o in outs]
    got, _ = f.run(world["batch"], world["fb"], 10, outs=outs)
    assert all(np.array_equal(a, b) for a, b in zip(first, got))
    # a flag that was set is written again
    outs[3].fill_(1)
    got, _ = f.run(world["batch"], world["fb"], 10, outs=outs)
    assert int(got[3][0]) == 0


def test_many_queries(world):
    """More queries than one workgroup of the compaction owns: 600 copies with rotated feedback lists"""
    q_ptr, q_term, q_weight = world["batch"]
    reps = 19
    lens = np.tile(np.diff(q_ptr), reps)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    fb = tuple(np.roll(np.concatenate([x] * reps), 7, axis=0) for x in world["fb"])
    exp, _ = world["fwd"].check((p, np.tile(q_term, reps), np.tile(q_weight, reps)), fb, 10, label="627 queries")
    assert len(exp[0]) == NQ * reps + 1 > 513


# ---- end to end: the doors on tests/golden/text_small.json ------------------------------------------------------------------------
class _Text:
    """The golden text corpus as host arrays, the oracle's full rankings and the restated two-pass search"""

    def __init__(self, corpus, queries):
        import sparse_rx
        self.corpus, self.queries = corpus, queries
        self.h = h = sparse_rx.build_host_index(self.corpus)
        self.n = h.n_docs
        self.rows = feedback_ref.forward_rows(h.indptr, h.indices, h.data, h.idf)
        self.gain = np.maximum(h.idf, 0).astype(np.float32)
        self.qids = [q for q, t in self.queries.items() if t and t.strip()]
        self.batch = sparse_rx.encode_queries([self.queries[q] for q in self.qids], h.vocabulary)

    def ranking(self, batch, keep, k):
        """The oracle's ranking of every query of ``batch`` restricted to the doc rows ``keep[i]`` (None: all), cut to k ->
        (doc [nq, k] padded with -1, score, count)"""
        import oracle
        h = self.h
        d, s, c = oracle.search_batch(h.indptr, h.indices, h.data, h.doc_lengths, h.idf, *batch, self.n, 1.2, 0.75, h.avgdl)
        nq = len(batch[0]) - 1
        od, os_, oc = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
        for i in range(nq):
            rows = [(int(d[i, j]), s[i, j]) for j in range(int(c[i])) if keep is None or keep[i] is None or int(d[i, j]) in keep[i]][:k]
            oc[i] = len(rows)
            od[i, : len(rows)] = [r[0] for r in rows]
            os_[i, : len(rows)] = [r[1] for r in rows]
        return od, os_, oc

    def two_pass(self, keep, k, R, n_terms=10, weight=0.5):
        """{qid: {doc_id: score}} of the restated expansion of the oracle's own first pass, searched by the oracle"""
        first = self.ranking(self.batch, keep, R)
        rp, tm, vl, longest = self.rows
        e = feedback_ref.expand(rp, tm, vl, self.h.doc_lengths, self.n, 0, R, max(1, min(longest, 4096 // R)), n_terms, BY_SCORE, RM, 1.0 - weight, weight,
                                self.gain, *self.batch, *first)
        d, s, c = self.ranking(e[:3], keep, k)
        ids = self.h.doc_ids
        out = {q: {} for q in self.queries}
        for i, q in enumerate(self.qids):
            out[q] = {ids[int(d[i, j])]: float(s[i, j]) for j in range(int(c[i]))}
        return out, first, e


@pytest.fixture(scope="module")
def text(golden_dir):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    return _Text(j["corpus"], j["queries"])


def _same(got, exp, label):
    assert list(got) == list(exp), label
    for q in exp:
        assert list(got[q].items()) == list(exp[q].items()), (label, q)


def test_search_bm25_expanded_is_the_oracle_of_the_restated_expansion(text):
    import sparse_rx
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(text.corpus)
    with pytest.raises(ValueError, match=r"search_bm25\(expand_docs=\.\.\.\) needs the forward index: call enable_feedback\(\) first"):
        svc.search_bm25(text.queries, top_k=10, expand_docs=5)
    svc.enable_feedback()
    plain = svc.search_bm25(text.queries, top_k=10)
    cached = len(svc.query_cache)
    got = svc.search_bm25(text.queries, top_k=10, expand_docs=5)
    exp, _, _ = text.two_pass(None, 10, 5)
    _same(got, exp, "expand_docs=5")
    assert len(svc.query_cache) == cached  # the expanded call neither read nor wrote the cache
    assert sum(list(got[q]) != list(plain[q]) for q in text.qids) > len(text.qids) // 2  # the expansion changes what is found
    assert svc.search_bm25(text.queries, top_k=10) == plain
    _same(svc.search_bm25(text.queries, top_k=7, expand_docs=32, expand_terms=3, expand_weight=0.9), text.two_pass(None, 7, 32, 3, 0.9)[0], "R=32")
    _same(svc.search_bm25(text.queries, top_k=10, expand_docs=5, expand_weight=0.0), text.two_pass(None, 10, 5, 10, 0.0)[0], "weight 0")
    _same(svc.search_bm25(text.queries, top_k=text.n, expand_docs=5), text.two_pass(None, text.n, 5)[0], "whole corpus")
    # under excluded_docs= and where=: both passes see the allowed docs alone
    ids = text.h.doc_ids
    shown = [d for q in text.qids[:6] for d in list(plain[q])[:3]]
    keep = set(range(text.n)) - {ids.index(d) for d in shown}
    _same(svc.search_bm25(text.queries, top_k=10, expand_docs=5, excluded_docs=shown), text.two_pass([keep] * len(text.qids), 10, 5)[0], "excluded_docs")
    year = (np.arange(text.n) * 7 % 24 + 2000).astype(np.int32)
    svc.set_doc_fields({"year": year, "group": (np.arange(text.n) // 4).astype(np.int32)})
    keep = set(np.nonzero(year >= 2008)[0].tolist())
    got = svc.search_bm25(text.queries, top_k=10, expand_docs=5, where={"must": [{"field": "year", "gte": 2008}]})
    _same(got, text.two_pass([keep] * len(text.qids), 10, 5)[0], "where")
    # collapse_by= applies to the second pass only: the collapsed ranking of the expanded query
    full = text.two_pass(None, text.n, 5)[0]
    got = svc.search_bm25(text.queries, top_k=10, expand_docs=5, collapse_by="group")
    for q in text.qids:
        seen, want = set(), []
        for d in full[q]:
            g = ids.index(d) // 4
            if g not in seen:
                seen.add(g)
                want.append(d)
        assert list(got[q]) == want[:10] and all(got[q][d] == full[q][d] for d in got[q]), q
    # what the queries were expanded to: the batch of the second pass, by words
    words = svc.expand_queries(text.queries, {q: dict(list(plain[q].items())[:5]) for q in text.queries})
    _, _, e = text.two_pass(None, 10, 5)
    inv = {t: w for w, t in text.h.vocabulary.items()}
    for i, q in enumerate(text.qids):
        assert list(words[q].items()) == [(inv[int(t)], float(w)) for t, w in zip(e[1][e[0][i]: e[0][i + 1]], e[2][e[0][i]: e[0][i + 1]])], q
        total = sum(words[q].values())  # at most 1; exactly alpha + beta = 1 when the query has terms and feedback docs
        assert total <= 1.0 + 1e-5 and (not plain[q] or abs(total - 1.0) < 1e-5), q
    svc.close()
    with pytest.raises(ValueError, match="enable_feedback"):
        svc.search_bm25(text.queries, top_k=10, expand_docs=5)


def test_registry_doors(text, tmp_path):
    import sparse_rx
    exp, _, _ = text.two_pass(None, 10, 5)
    r = sparse_rx.OptimizedBM25Retriever(device=DEVICE, tile_log2=6)
    r.build_index_from_corpus(text.corpus)
    r.enable_feedback()
    _same(r.search(text.queries, top_k=10, expand_docs=5), exp, "OptimizedBM25Retriever")
    r.close()
    r = sparse_rx.OptimizedRetriever({"type": "bm25"}, device=DEVICE, tile_log2=6, cache_dir=str(tmp_path), accumulation="term")
    r.build_index_from_corpus(text.corpus)
    r.enable_feedback()
    _same(r.search(text.queries, top_k=10, expand_docs=5), exp, "OptimizedRetriever")
    r.close()
    # dot mode: raw values, every gain 1 -- against the oracle's dot mode
    import oracle
    r = sparse_rx.OptimizedRetriever({"type": "tfidf"}, device=DEVICE, tile_log2=6, cache_dir=str(tmp_path), accumulation="term")
    r.build_index_from_corpus(text.corpus)
    r.enable_feedback()
    h = r.host
    qids = [q for q, t in text.queries.items() if t]
    batch = sparse_rx.encode_queries([text.queries[q] for q in qids], h.vocabulary)
    search = lambda b, k: oracle.search_batch(h.indptr, h.indices, h.data, None, h.idf, *b, k, mode=oracle.MODE_TFIDF_F32)
    rp, tm, vl, longest = feedback_ref.forward_rows(h.indptr, h.indices, h.data, h.idf)
    e = feedback_ref.expand(rp, tm, vl, None, h.n_docs, 0, 5, max(1, min(longest, 4096 // 5)), 10, BY_SCORE, RAW, 0.5, 0.5, None, *batch, *search(batch, 5))
    d, s, c = search(e[:3], 10)
    got = r.search(text.queries, top_k=10, expand_docs=5)
    for i, q in enumerate(qids):
        assert list(got[q].items()) == [(h.doc_ids[int(d[i, j])], float(s[i, j])) for j in range(int(c[i])) if s[i, j] > 0], q
    r.close()


def test_more_like_this(text):
    import sparse_rx
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(text.corpus)
    svc.enable_feedback()
    ids = text.h.doc_ids
    seeds = {"a": [ids[3], ids[70], ids[200]], "b": [ids[5]], "none": [], "c": [ids[i] for i in range(100, 132)]}
    rp, tm, vl, longest = text.rows
    live = [q for q in seeds if seeds[q]]
    m = max(len(v) for v in seeds.values())
    fb_doc = np.full((len(seeds), m), -1, np.int32)
    for i, q in enumerate(seeds):
        fb_doc[i, : len(seeds[q])] = [ids.index(d) for d in seeds[q]]
    count = np.asarray([len(v) for v in seeds.values()], np.int32)
    empty = (np.zeros(len(seeds) + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    e = feedback_ref.expand(rp, tm, vl, text.h.doc_lengths, text.n, 0, m, max(1, min(longest, 4096 // m)), 25, UNIFORM, RM, 0.0, 1.0, text.gain, *empty,
                            fb_doc, np.zeros(fb_doc.shape, np.float32), count)
    assert np.diff(e[0]).tolist() == [25, 25, 0, 25]
    for include in (False, True):
        keep = [None if include else set(range(text.n)) - set(fb_doc[i, : count[i]].tolist()) for i in range(len(seeds))]
        d, s, c = text.ranking(e[:3], keep, 10)
        got = svc.more_like_this(seeds, top_k=10, include_seeds=include)
        assert list(got) == list(seeds) and got["none"] == {}
        for i, q in enumerate(seeds):
            assert list(got[q].items()) == [(ids[int(d[i, j])], float(s[i, j])) for j in range(int(c[i]))], (q, include)
            assert include or not set(got[q]) & set(seeds[q])
    assert set(seeds["b"]) & set(svc.more_like_this(seeds, top_k=10, include_seeds=True)["b"])  # a doc is most like itself
    # the doc keywords: the caller's exclude list joins the seeds, an allow list loses them
    hidden = list(svc.more_like_this(seeds, top_k=10)["a"])[:4]
    gone = {ids.index(d) for d in hidden}
    keep = [set(range(text.n)) - set(fb_doc[i, : count[i]].tolist()) - gone for i in range(len(seeds))]
    d, s, c = text.ranking(e[:3], keep, 10)
    got = svc.more_like_this(seeds, top_k=10, excluded_docs=hidden)
    for i, q in enumerate(seeds):
        assert list(got[q].items()) == [(ids[int(d[i, j])], float(s[i, j])) for j in range(int(c[i]))], q
    allowed = ids[:150]
    keep = [set(range(150)) - set(fb_doc[i, : count[i]].tolist()) for i in range(len(seeds))]
    d, s, c = text.ranking(e[:3], keep, 10)
    got = svc.more_like_this(seeds, top_k=10, allowed_docs=allowed)
    for i, q in enumerate(seeds):
        assert list(got[q].items()) == [(ids[int(d[i, j])], float(s[i, j])) for j in range(int(c[i]))], q
    with pytest.raises(ValueError, match="must name every qid"):
        svc.more_like_this(seeds, allowed_docs={"a": allowed})
    with pytest.raises(ValueError, match="at most 32 seeds"):
        svc.more_like_this({"x": ids[:33]})
    with pytest.raises(ValueError, match="unknown doc id 'nope'"):
        svc.more_like_this({"x": ["nope"]})
    svc.close()


def test_planted_cooccurrence():
    """A always co-occurs with B; one doc holds B without A.  The query for A finds it after expansion and not before."""
    import sparse_rx
    rng = np.random.default_rng(4)
    filler = lambda: " ".join(f"w{int(x)}" for x in rng.integers(0, 400, 12))
    corpus = {f"d{i}": {"text": filler()} for i in range(120)}
    for i in range(0, 24, 2):
        corpus[f"d{i}"]["text"] += " alpha beta beta"
    corpus["only_b"] = {"text": filler() + " beta beta"}
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(corpus)
    svc.enable_feedback()
    q = {"q": "alpha"}
    before = svc.search_bm25(q, top_k=50)["q"]
    after = svc.search_bm25(q, top_k=50, expand_docs=10, expand_terms=5)["q"]
    assert len(before) == 12 and "only_b" not in before and "only_b" in after
    assert "beta" in svc.expand_queries(q, {"q": dict(list(before.items())[:10])}, expand_terms=5)["q"]
    svc.close()


def test_deeper_than_the_lists():
    """top_k above the engine's 1 024-row lists: the expanded batch goes to the host once and takes the paged route"""
    import sparse_rx
    rng = np.random.default_rng(6)
    corpus = {f"d{i}": {"text": " ".join(f"w{int(x)}" for x in rng.integers(0, 30, 12))} for i in range(1300)}
    t = _Text(corpus, {"q0": "w1 w2", "q1": "w7", "q2": ""})
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=8)
    svc.build_bm25_index(corpus)
    svc.enable_feedback()
    got = svc.search_bm25(t.queries, top_k=1200, expand_docs=10, expand_terms=5)
    _same(got, t.two_pass(None, 1200, 10, 5)[0], "top_k=1200")
    assert len(got["q0"]) > 1024 and got["q2"] == {}
    svc.close()
