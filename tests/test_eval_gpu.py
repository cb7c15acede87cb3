"""``srx_eval_lists`` on the GPU, BIT FOR BIT against the fp32 restatement of tests/eval_ref.py: every plane, every word, the means
included, at the smallest shapes that reach each edge of the two kernels -- the wave / workgroup switch in m, the LDS row capacity,
a mean chunk -- with the outputs poisoned before every call.

Every test here needs ``sparse_rx.Judgments`` or ``srx_eval_lists``: without the feature the whole file fails."""
import ctypes
import json
import os

import numpy as np
import pytest

import eval_ref
from test_eval_cpu import random_case, refusals

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"
N_DOCS = 40000
ROW_LENS = [0, 1, eval_ref.LDS_ROW - 1, eval_ref.LDS_ROW, eval_ref.LDS_ROW + 1, 20000, 3, 17, 64, 300]  # both join paths in one launch


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch


@pytest.fixture(scope="module")
def rows():
    """the judgment rows every shape test shares: grades from -2 (judged, non-relevant) to 40 (above every table)"""
    rng = np.random.default_rng(11)
    j_ptr = np.concatenate([[0], np.cumsum(ROW_LENS)]).astype(np.int64)
    j_doc = np.concatenate([np.sort(rng.choice(N_DOCS, n, replace=False)) for n in ROW_LENS]).astype(np.int32)
    j_grade = rng.integers(-2, 41, len(j_doc)).astype(np.int32)
    j_grade[rng.random(len(j_doc)) < 0.5] = 0
    return dict(j_ptr=j_ptr, j_doc=j_doc, j_grade=j_grade, j_ideal=eval_ref.ideal_of(j_ptr, j_grade))


def lists_for(rng, rows, q_row, m):
    """lists that hit their rows: half the positions from the row (its first and last doc first), the rest anywhere -- negative ids,
    ids above every judged one, docs twice"""
    nq = len(q_row)
    cand = rng.integers(-5, N_DOCS + 50, (nq, m)).astype(np.int32)
    for q, r in enumerate(q_row):
        if 0 <= r < len(ROW_LENS) and ROW_LENS[r]:
            docs = rows["j_doc"][rows["j_ptr"][r]:rows["j_ptr"][r + 1]]
            take = rng.random(m) < 0.5
            cand[q, take] = rng.choice(docs, int(take.sum()))
            cand[q, 0] = docs[0]
            cand[q, m - 1] = docs[-1]
    return cand


def cutoffs(m, n_k):
    return [m + 5] if n_k == 1 else sorted({1, 3, 64, 65, m, m + 1, 1500, 25000})[:8]


def gpu_eval(torch, rows, gain, discount, rel_level, cand, count, q_row, ks, means=True, n_rows=None):
    """one call through the C ABI, every output poisoned with 0xFF bytes first -> the dict eval_ref.eval_lists returns"""
    from sparse_rx import _capi
    dev = torch.device(DEVICE)
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    j = [up(rows[n]) for n in ("j_ptr", "j_doc", "j_grade", "j_ideal")]
    g, d, c, cnt, qr = up(np.asarray(gain, np.float32)), up(np.asarray(discount, np.float32)), up(cand), up(count), up(q_row)
    nq, m = cand.shape
    n_k = len(ks)
    poison = lambda shape, dtype: torch.full(shape, -1, dtype=dtype, device=dev)
    out, hits, judged, rel = poison((nq, n_k, 8), torch.int32), poison((nq, n_k), torch.int32), poison((nq, n_k), torch.int32), poison((nq,), torch.int32)
    mean, n = (poison((n_k, 8), torch.int64), poison((1,), torch.int32)) if means else (None, None)
    L = _capi.lib()
    ws_bytes = L.srx_eval_workspace_bytes(nq, n_k) if means else 0
    ws = poison((max(ws_bytes // 8, 1),), torch.int64) if means else None
    rc = L.srx_eval_lists(0, *[ptr(t) for t in j], len(rows["j_ptr"]) - 1 if n_rows is None else n_rows, len(rows["j_doc"]), ptr(g), len(gain), ptr(d),
                          rel_level, ptr(c), ptr(cnt), ptr(qr), nq, m, (ctypes.c_int32 * n_k)(*ks), n_k, ptr(out), ptr(hits), ptr(judged), ptr(rel),
                          ptr(mean), ptr(n), ptr(ws), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
    _capi.check(rc, "srx_eval_lists")
    torch.cuda.synchronize(dev)
    res = {"out": out.cpu().numpy().view(np.float32), "hits": hits.cpu().numpy(), "judged": judged.cpu().numpy(), "rel": rel.cpu().numpy()}
    if means:
        res["mean"], res["n"] = mean.cpu().numpy().view(np.float64), int(n.cpu().numpy()[0])
    return res


def same_bits(got, want, what=""):
    assert np.array_equal(got["hits"], want["hits"]), f"{what}: hits"
    assert np.array_equal(got["judged"], want["judged"]), f"{what}: judged"
    assert np.array_equal(got["rel"], want["rel"]), f"{what}: rel"
    bad = np.argwhere(got["out"].view(np.uint32) != want["out"].view(np.uint32))
    assert len(bad) == 0, f"{what}: out differs at (q, cutoff, metric) {bad[:5].tolist()}: {[(got['out'][tuple(b)], want['out'][tuple(b)]) for b in bad[:5]]}"
    if "mean" in want:
        assert got["n"] == want["n"], f"{what}: n"
        assert np.array_equal(got["mean"].view(np.uint64), want["mean"].view(np.uint64)), f"{what}: means {got['mean']} != {want['mean']}"


def check(torch, rows, gain_kind, n_gain, rel_level, cand, count, q_row, ks, means=True, n_rows=None, what=""):
    gain, discount = eval_ref.gain_table(gain_kind, n_gain), eval_ref.discount_table(cand.shape[1])
    got = gpu_eval(torch, rows, gain, discount, rel_level, cand, count, q_row, ks, means, n_rows)
    r = rows if n_rows is None else dict(rows, j_ptr=rows["j_ptr"][:n_rows + 1])
    want = eval_ref.eval_lists(r["j_ptr"], r["j_doc"], r["j_grade"], r["j_ideal"], gain, discount, rel_level, cand, count, q_row, ks, means,
                               nnz=len(rows["j_doc"]))
    same_bits(got, want, what)
    return got


M_EDGES = [1, 63, 64, 65, eval_ref.WAVE_M, eval_ref.WAVE_M + 1, 2047, 2048]  # 256 / 257: the two sides of the wave / workgroup switch


@pytest.mark.parametrize("nq", [1, 5, 1025])  # 1025 crosses a mean chunk
@pytest.mark.parametrize("m", M_EDGES)
def test_shapes(torch, rows, m, nq):
    i = M_EDGES.index(m) * 3 + [1, 5, 1025].index(nq)
    rng = np.random.default_rng(100 + i)
    n_rows = len(ROW_LENS)
    q_row = [None, rng.integers(-1, n_rows + 2, nq).astype(np.int32), rng.permutation(np.arange(nq) % n_rows).astype(np.int32)][i % 3]
    rows_of = np.arange(nq) if q_row is None else q_row  # NULL: identity; a list past the last row is not judged
    cand = lists_for(rng, rows, rows_of, m)
    count = [None, rng.integers(-2, m + 3, nq).astype(np.int32)][(i // 3) % 2]
    if count is not None and nq >= 5:
        count[:5] = [0, -7, m, m + 9, max(m // 2, 1)]
    n_gain, gain_kind, rel_level = [2, 5, 32][i % 3], ["linear", "exp2"][(i // 2) % 2], 1 + (i // 4) % 2
    got = check(torch, rows, gain_kind, n_gain, rel_level, cand, count, q_row, cutoffs(m, 1 if i % 4 == 3 else 8), what=f"m={m} nq={nq}")
    assert got["n"] == int(((rows_of >= 0) & (rows_of < n_rows)).sum())
    if nq == 1025:  # 32 grades there: something is relevant whatever the level
        assert got["hits"].any() and got["judged"].any() and got["out"][:, :, eval_ref.NDCG].any()


@pytest.mark.parametrize("m", [64, 300])
def test_every_row_length_on_both_kernels(torch, rows, m):
    """one list per row length -- 0, 1, the LDS capacity - 1, the capacity, the capacity + 1, 20 000 -- with repeats: the staged and the
    global join in one launch; gains of 2, 5 and 32 grades, both gain kinds, both levels"""
    rng = np.random.default_rng(5)
    q_row = np.asarray(list(range(len(ROW_LENS))) + [5, 4, 3, 5, 0], dtype=np.int32)
    cand = lists_for(rng, rows, q_row, m)
    for n_gain in (2, 5, 32):
        for gain_kind in ("linear", "exp2"):
            for rel_level in (1, 2):
                got = check(torch, rows, gain_kind, n_gain, rel_level, cand, None, q_row, [1, 10, m, 30000], what=f"{gain_kind} {n_gain} {rel_level}")
    assert got["rel"][5] > 1000 and got["rel"][0] == 0 and got["hits"][5, 2] > 3 and got["hits"][3, 2] > 3


def test_counts_and_cutoffs(torch, rows):
    rng = np.random.default_rng(6)
    m = 130
    q_row = np.asarray([5, 3, 8, 1, 6, 0, 9], dtype=np.int32)
    cand = lists_for(rng, rows, q_row, m)
    for count in (None, [0] * 7, [-1, -100, 0, 1, 2, 3, 4], [m] * 7, [m + 1, 2 ** 31 - 1, m, m - 1, 64, 65, 63]):
        cnt = None if count is None else np.asarray(count, dtype=np.int32)
        check(torch, rows, "exp2", 5, 1, cand, cnt, q_row, [7], what=f"count {count}")                       # n_k = 1
        check(torch, rows, "linear", 5, 1, cand, cnt, q_row, [1, 2, 4, 64, 129, 130, 131, 2 ** 31 - 1], what=f"count {count}")  # n_k = 8, above m
    check(torch, rows, "linear", 5, 1, cand, None, q_row, [m + 1], means=False)


def test_rows_of_queries(torch, rows):
    rng = np.random.default_rng(8)
    m, nq, n_rows = 40, 1030, len(ROW_LENS)
    for q_row in (None, np.full(nq, -1, np.int32), np.full(nq, n_rows, np.int32), rng.integers(-3, n_rows + 3, nq).astype(np.int32),
                  np.full(nq, 5, np.int32)):
        rows_of = np.arange(nq) if q_row is None else q_row
        got = check(torch, rows, "linear", 5, 1, lists_for(rng, rows, rows_of, m), None, q_row, [5, 40], what=f"q_row {None if q_row is None else q_row[:4]}")
    got = check(torch, rows, "linear", 5, 1, lists_for(rng, rows, np.full(7, -1), m), None, np.full(7, -1, np.int32), [5, 40])
    assert got["n"] == 0 and not got["mean"].view(np.uint64).any() and not got["out"].view(np.uint32).any()  # all unjudged: +0 everywhere
    # no judged query at all (n_rows = 0), and fewer rows than the arrays hold
    check(torch, rows, "linear", 5, 1, lists_for(rng, rows, np.arange(4), m), None, None, [5], n_rows=0)
    check(torch, rows, "linear", 5, 1, lists_for(rng, rows, np.arange(9), m), None, None, [5], n_rows=6)


def test_same_query_at_different_places(torch, rows):
    """no grid hint is exposed, so: one query alone, then inside batches of other sizes at other positions (another wave of its
    workgroup, another workgroup) -- its words do not change.  Both kernels."""
    rng = np.random.default_rng(9)
    for m in (200, 700):
        q_row = rng.integers(0, len(ROW_LENS), 300).astype(np.int32)
        q_row[[0, 2, 257]] = 5
        cand = lists_for(rng, rows, q_row, m)
        cand[2], cand[257] = cand[0], cand[0]
        ks = [1, 10, 100, 1000]
        alone = check(torch, rows, "exp2", 5, 1, cand[:1], None, q_row[:1], ks)
        batch = check(torch, rows, "exp2", 5, 1, cand, None, q_row, ks)
        small = check(torch, rows, "exp2", 5, 1, cand[:3], None, q_row[:3], ks)
        for res, q in ((batch, 0), (batch, 2), (batch, 257), (small, 2)):
            assert np.array_equal(res["out"][q].view(np.uint32), alone["out"][0].view(np.uint32)) and np.array_equal(res["hits"][q], alone["hits"][0])


def test_random_rows(torch):
    """rows and lists drawn like the CPU test's: many small rows, lists without repeats, every count"""
    rng = np.random.default_rng(12)
    c = random_case(rng, 2000, 24, n_rows=400, max_row=30, n_docs=60, grades=(-1, 5))
    check(torch, c, "exp2", 5, 2, c["cand_doc"], c["cand_count"], c["q_row"], [1, 3, 10, 30])


def test_refusals_on_the_gpu_machine():
    refusals()


def test_judgments_doors(torch, rows):
    import sparse_rx
    rng = np.random.default_rng(13)
    r = np.repeat(np.arange(len(ROW_LENS)), ROW_LENS)
    j = sparse_rx.Judgments.from_arrays(r, rows["j_doc"], rows["j_grade"], n_rows=len(ROW_LENS), device=DEVICE)
    assert np.array_equal(j.j_ptr, rows["j_ptr"]) and np.array_equal(j.j_doc, rows["j_doc"]) and np.array_equal(j.j_ideal, rows["j_ideal"]) and j.n_gain == 32
    q_row = rng.integers(-1, len(ROW_LENS), 50).astype(np.int32)
    cand, count, ks = lists_for(rng, rows, q_row, 90), rng.integers(0, 91, 50).astype(np.int32), [1, 10, 100]
    dev = torch.device(DEVICE)
    res = j.evaluate_device(torch.as_tensor(cand, device=dev), torch.as_tensor(count, device=dev), ks, torch.as_tensor(q_row, device=dev), gain="exp2", rel_level=2,
                            n_gain=6)
    assert all(t.device == dev for t in res) and res.mean.dtype == torch.float64 and tuple(res.out.shape) == (50, 3, 8)
    want = eval_ref.eval_lists(rows["j_ptr"], rows["j_doc"], rows["j_grade"], rows["j_ideal"], eval_ref.gain_table("exp2", 6), eval_ref.discount_table(90), 2,
                               cand, count, q_row, ks)
    got = {"out": res.out.cpu().numpy(), "hits": res.hits.cpu().numpy(), "judged": res.judged.cpu().numpy(), "rel": res.rel.cpu().numpy(),
           "mean": res.mean.cpu().numpy(), "n": int(res.n.cpu()[0])}
    same_bits(got, want, "evaluate_device")
    host = j.evaluate(cand, count, ks, q_row, gain="exp2", rel_level=2, n_gain=6)
    same_bits(host._asdict(), want, "evaluate")
    plain = j.evaluate(cand, ks=ks, means=False)  # defaults: linear gains over 32 grades, every position live, list q = row q
    assert plain.mean is None and plain.n is None
    want = eval_ref.eval_lists(rows["j_ptr"], rows["j_doc"], rows["j_grade"], rows["j_ideal"], eval_ref.gain_table("linear", 32), eval_ref.discount_table(90), 1,
                               cand, None, None, ks, means=False)
    same_bits(plain._asdict(), want, "evaluate, defaults")
    assert len(j._tables) == 2  # cached per (gain, n_gain, m)
    empty = j.evaluate(np.zeros((0, 4), np.int32), ks=[1])
    assert empty.out.shape == (0, 1, 8) and empty.n == 0 and not empty.mean.any()
    for bad, word in ((dict(doc=torch.zeros((2, 3), dtype=torch.int64, device=dev)), "doc must be"), (dict(doc=torch.zeros((2, 2049), dtype=torch.int32, device=dev)), "2048"),
                      (dict(count=torch.zeros((3,), dtype=torch.int32, device=dev)), "count must be"), (dict(rel_level=0), "rel_level"), (dict(ks=[2, 1]), "k_values"),
                      (dict(gain="log"), "gain must be")):
        args = dict(doc=torch.zeros((2, 3), dtype=torch.int32, device=dev), count=None, ks=[1])
        args.update(bad)
        with pytest.raises(ValueError, match=word):
            j.evaluate_device(**args)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        return json.load(f)


def planted(results, n_ghosts=2):
    """judgments planted on a ranking: every third doc of each list, grades 0 .. 3, plus docs that are not in the corpus"""
    qrels = {}
    for qi, (qid, row) in enumerate(results.items()):
        qrels[qid] = {d: (qi + i) % 4 for i, d in enumerate(row) if i % 3 == 0}
        for g in range(n_ghosts if qi % 2 else 0):
            qrels[qid][f"ghost-{g}"] = 1 + g
    qrels["never-searched"] = {"ghost-0": 1}
    return qrels


def test_search_then_evaluate_end_to_end(torch, text):
    import sparse_rx
    queries = {q: text["queries"][q] for q in list(text["queries"])[:12]}
    svc = sparse_rx.RetrievalService(device=DEVICE, tile_log2=6)
    svc.build_bm25_index(text["corpus"])
    deep = svc.search_bm25(queries, top_k=30)
    qrels = planted(deep)
    ks = (1, 3, 5, 10, 100)
    agg, per = svc.evaluate(qrels, svc.search_bm25(queries, top_k=20), ks, per_query=True)
    found = [q for q in queries if deep[q]]
    assert agg["n_queries"] == len(queries) and 0.0 < agg["NDCG@10"] < 1.0 and agg["Judged@1"] == len(found) / len(queries)
    # the same lists straight from the device: search_device -> evaluate_device, nothing else in between
    qids = list(queries)
    h = svc.host
    qp, qt, qw = sparse_rx.encode_queries([queries[q] for q in qids], h.vocabulary)
    dev = torch.device(DEVICE)
    doc, score, count = svc.dev.search_device(*[torch.as_tensor(a, device=dev) for a in (qp, qt, qw)], 20)
    j = sparse_rx.Judgments.from_qrels(qrels, None, h.doc_ids, device=DEVICE)
    assert j.extra_ids == {"ghost-0": h.n_docs, "ghost-1": h.n_docs + 1}
    res = j.evaluate_device(doc, count, ks, torch.as_tensor(np.asarray([j.row_of[q] for q in qids], np.int32), device=dev))
    out, mean = res.out.cpu().numpy(), res.mean.cpu().numpy()
    assert int(res.n.cpu()[0]) == agg["n_queries"]
    for ik, k in enumerate(ks):
        for name, plane in sparse_rx.evaluate.METRIC_KEYS:
            assert agg[f"{name}@{k}"] == float(mean[ik, plane]), (name, k)
            assert [per[q][f"{name}@{k}"] for q in qids] == [float(v) for v in out[:, ik, plane]], (name, k)
    # a Judgments built once serves every call; complete adds the judged query that was never searched; rank_eval is search + evaluate
    assert svc.evaluate(j, svc.search_bm25(queries, top_k=20), ks) == agg
    full = svc.evaluate(qrels, svc.search_bm25(queries, top_k=20), ks, complete=True)
    assert full["n_queries"] == agg["n_queries"] + 1 and full["P@5"] == pytest.approx(agg["P@5"] * agg["n_queries"] / full["n_queries"], rel=1e-12)
    assert svc.rank_eval(queries, qrels, (1, 3, 5, 10, 20)) == svc.evaluate(qrels, svc.search_bm25(queries, top_k=20), (1, 3, 5, 10, 20))
    kw = dict(excluded_docs=list(deep[found[0]])[:2])
    assert svc.rank_eval(queries, qrels, (5, 10), gain="exp2", rel_level=2, **kw) == svc.evaluate(qrels, svc.search_bm25(queries, top_k=10, **kw), (5, 10), gain="exp2",
                                                                                                 rel_level=2)
    retr = sparse_rx.OptimizedBM25Retriever(device=DEVICE, tile_log2=6)
    retr.build_index_from_corpus(text["corpus"])
    assert retr.rank_eval(queries, qrels, (1, 10)) == retr.evaluate(qrels, retr.search(queries, top_k=10), (1, 10))
    svc.close()


def test_merged_lists_of_two_shards(torch):
    """A sharded index is not refused: two doc-range shards on one GPU, each behind a ShardedSearcher without a process group (no
    collective runs), their lists merged by srx_merge_topk -- GLOBAL ids, evaluated like the lists of the whole index."""
    import sparse_rx
    from sparse_rx import synth
    from sparse_rx.index import merge_topk_device
    c = synth.uniform_corpus_np(6000, 800, 20, seed=3)
    _, idf, avgdl = synth.corpus_stats(c)
    q = synth.queries_np(40, c.vocab, 5, seed=4)
    dev = torch.device(DEVICE)
    dq = [torch.as_tensor(a, device=dev) for a in q]
    k = 50
    whole = sparse_rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, device=DEVICE, tile_log2=10)
    wd, ws, wc = whole.search_device(*dq, k)
    parts = []
    for rank in range(2):
        a, b = sparse_rx.shard_range(6000, 2, rank)
        ptr = c.indptr[a:b + 1] - c.indptr[a]
        sl = slice(int(c.indptr[a]), int(c.indptr[b]))
        ix = sparse_rx.DeviceIndex.from_csr(ptr, c.indices[sl], c.data[sl], idf, doc_lengths=c.doc_lengths[a:b], avgdl=avgdl, device=DEVICE, tile_log2=10,
                                            doc_base=a)
        parts.append((ix, sparse_rx.ShardedSearcher.for_device_index(ix).search(*dq, k)))
    md, ms, mc = merge_topk_device(torch.stack([p[1][0] for p in parts]), torch.stack([p[1][1] for p in parts]), torch.stack([p[1][2] for p in parts]), k,
                                   gathered=True)
    live = torch.arange(k, device=dev)[None, :] < wc[:, None]
    assert torch.equal(mc, wc) and torch.equal(md[live], wd[live]) and int(md.max()) >= 3000
    md = torch.where(live, md, wd)  # whatever pads a row
    rng = np.random.default_rng(5)
    host_doc, host_cnt = wd.cpu().numpy(), wc.cpu().numpy()
    rows_, docs_, grades_ = [], [], []
    for qi in range(40):  # judgments planted on both shards' docs, and on docs never retrieved
        picked = np.unique(np.concatenate([host_doc[qi, :host_cnt[qi]][::4], rng.integers(0, 6000, 5)]))
        rows_ += [qi] * len(picked)
        docs_ += picked.tolist()
        grades_ += rng.integers(0, 4, len(picked)).tolist()
    j = sparse_rx.Judgments.from_arrays(rows_, docs_, grades_, n_rows=40, device=DEVICE)
    ks = [1, 10, 50]
    merged, single = j.evaluate_device(md, mc, ks), j.evaluate_device(wd, wc, ks)
    for a, b in zip(merged, single):
        assert torch.equal(a, b)
    want = eval_ref.eval_lists(j.j_ptr, j.j_doc, j.j_grade, j.j_ideal, eval_ref.gain_table("linear", j.n_gain), eval_ref.discount_table(k), 1, host_doc, host_cnt,
                               None, ks)
    same_bits({"out": merged.out.cpu().numpy(), "hits": merged.hits.cpu().numpy(), "judged": merged.judged.cpu().numpy(), "rel": merged.rel.cpu().numpy(),
               "mean": merged.mean.cpu().numpy(), "n": int(merged.n.cpu()[0])}, want, "merged shards")
    assert want["hits"][:, 2].sum() > 100
    for ix, _ in parts:
        ix.close()
    whole.close()
