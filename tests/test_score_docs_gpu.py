"""srx_score_docs on the MI355X: every entry of every output compared by its fp32 bits (``view(uint32)`` equality, no
tolerance, nothing skipped) with the reference-written score vectors of tests/golden or with ``oracle.scores_given_order``
on the host CSR, gathered at the candidates (tests/score_ref.py)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (checker only)
from score_ref import assert_bits_equal, gather_expected, oracle_full_scores  # noqa: E402


@pytest.fixture(scope="module")
def rx():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()  # fails loudly if the HIP library is missing
    return sparse_rx


def _rows(got, qids, doc_ids):
    return np.array([[got[q][d] for d in doc_ids] for q in qids], np.float32)


def _full(c, idf, avgdl, q, tfidf=False, k1=1.2, b=0.75):
    return oracle_full_scores(oracle, c.indptr, c.indices, c.data, c.doc_lengths, idf, q[0], q[1], q[2], k1, b, avgdl, tfidf=tfidf)


def _queries_of_lengths(lengths, vocab, seed, weights="count"):
    """A CSR batch whose query i has lengths[i] distinct terms in ascending order."""
    rng = np.random.default_rng(seed)
    q_ptr = np.zeros(len(lengths) + 1, np.int32)
    q_ptr[1:] = np.cumsum(lengths)
    terms = [np.sort(rng.choice(vocab, n, replace=False)).astype(np.int32) for n in lengths]
    q_term = np.concatenate(terms) if terms else np.zeros(0, np.int32)
    if weights == "count":
        q_w = np.where(rng.random(len(q_term)) < 0.1, 2.0, 1.0).astype(np.float32)
    else:
        q_w = (np.abs(rng.standard_normal(len(q_term))) + 0.05).astype(np.float16).astype(np.float32)
    return q_ptr, q_term, q_w


# ---------------------------------------------------------------------------------------------------------------
# 1. the reference's own score vectors, through the API mirrors and through DeviceIndex.from_csr
# ---------------------------------------------------------------------------------------------------------------
def test_reference_fixtures_through_the_mirrors(rx, golden_dir, tmp_path):
    z = np.load(os.path.join(golden_dir, "text_small.npz"))
    p = np.load(os.path.join(golden_dir, "pipeline_small.npz"))
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    doc_ids = [str(d) for d in z["doc_ids"]]
    qids = [str(q) for q in z["score_qids"]]
    queries = {q: j["queries"][q] for q in qids}
    for one_copy in (True, False):
        svc = rx.RetrievalService(device="cuda:0", tile_log2=6, one_copy=one_copy)
        svc.build_bm25_index(j["corpus"])
        got = svc.score_bm25(queries, {q: doc_ids for q in qids})
        assert list(got) == qids and all(list(got[q]) == doc_ids for q in qids)
        assert_bits_equal(_rows(got, qids, doc_ids), z["full_scores"], f"RetrievalService one_copy={one_copy}")
        # a search row scores to its own floats; ragged lists; blank / unknown
        top = svc.search_bm25(queries, top_k=10)
        again = svc.score_bm25(queries, {q: list(top[q]) for q in qids})
        assert again == top
        rag = svc.score_bm25({"a": queries[qids[0]], "b": "   ", "c": queries[qids[1]], "d": queries[qids[2]]},
                             {"a": doc_ids[3:4], "b": doc_ids[:5], "c": doc_ids[::-9], "d": []})
        assert rag["d"] == {} and rag["b"] == {d: 0.0 for d in doc_ids[:5]}
        assert rag["a"] == {doc_ids[3]: float(z["full_scores"][0, 3])}
        assert_bits_equal(np.array(list(rag["c"].values()), np.float32), z["full_scores"][1, ::-9], "ragged")
        with pytest.raises(ValueError, match="no-such-doc"):
            svc.score_bm25({"a": "w1"}, {"a": ["no-such-doc"]})
        svc.close()
    reg = rx.OptimizedBM25Retriever(device="cuda:0", tile_log2=7)
    reg.build_index_from_corpus(j["corpus"])
    assert_bits_equal(_rows(reg.score(queries, {q: doc_ids for q in qids}), qids, doc_ids), z["full_scores"], "OptimizedBM25Retriever")
    reg.close()
    for name, cfg in (("bm25", {"type": "bm25"}), ("splade", {"type": "splade"})):
        pq = [str(q) for q in p[f"{name}_qids"]]
        r = rx.OptimizedRetriever(cfg, device="cuda:0", tile_log2=6, accumulation="token", cache_dir=str(tmp_path / name))
        r.build_index_from_corpus(j["corpus"])
        got = r.score({q: j["queries"][q] for q in pq}, {q: doc_ids for q in pq})
        assert_bits_equal(_rows(got, pq, doc_ids), p[f"{name}_full_scores"], f"OptimizedRetriever {name} token order")
        r.close()


@pytest.mark.parametrize("tile_log2,unit_tiles,keep", [(9, 2, True), (8, 3, False), (12, 1, False), (6, 0, True)])
def test_csr_zipf_fixture(rx, golden_dir, tile_log2, unit_tiles, keep):
    z = np.load(os.path.join(golden_dir, "csr_zipf.npz"))
    n = int(z["tf_shape"][0])
    nq = z["bm25_full"].shape[0]
    q = (z["q_ptr"][: nq + 1], z["q_term"], z["q_weight"])
    cand = np.tile(np.arange(n, dtype=np.int32), (nq, 1))
    ix = rx.DeviceIndex.from_csr(z["tf_indptr"], z["tf_indices"], z["tf_data"], z["idf"], doc_lengths=z["doc_lengths"], k1=float(z["k1"]),
                                 b=float(z["b"]), avgdl=float(z["avgdl"]), tile_log2=tile_log2, unit_tiles=unit_tiles, keep_canonical=keep)
    assert_bits_equal(ix.score_docs(*q, cand), z["bm25_full"], "csr_zipf bm25")
    ix.close()
    for vd in ("f32", "f16"):  # the term counts are small integers: exact in fp16
        ix = rx.DeviceIndex.from_csr(z["tf_indptr"], z["tf_indices"], z["tf_data"], z["idf_tfidf"], mode="dot", val_dtype=vd,
                                     tile_log2=tile_log2, unit_tiles=unit_tiles, keep_canonical=keep)
        assert_bits_equal(ix.score_docs(*q, cand), z["tfidf_full"], f"csr_zipf dot {vd}")
        ix.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. value types x resident copies x tile sizes x corpora
# ---------------------------------------------------------------------------------------------------------------
def _mixed_candidates(rng, rows, n, G, U, m_random=40):
    """Per query: its own search rows (-1 padding included), random docs, the tile / unit / shard boundary docs,
    out-of-range ids, repeats."""
    d, _, _ = rows
    nq = d.shape[0]
    special = np.array([x for x in (0, G - 1, G, U - 1, U, n - 1) if 0 <= x < n] + [-1, -7, n, 2 ** 31 - 1], np.int64)
    rnd = rng.integers(0, n, size=(nq, m_random))
    block = np.concatenate([d.astype(np.int64), rnd, np.tile(special, (nq, 1)), rnd[:, :5], d[:, :3].astype(np.int64)], axis=1)
    return block.astype(np.int32)


@pytest.mark.parametrize("corpus", ["uniform", "zipf"])
@pytest.mark.parametrize("kind", ["bm25_f32", "dot_f32", "dot_f16"])
def test_matrix_of_layouts(rx, corpus, kind):
    from sparse_rx import synth
    n = 200_000
    if corpus == "uniform":
        c = synth.uniform_corpus_np(n, 20_000, 40, seed=411)
        q = synth.queries_np(24, c.vocab, 8, seed=412)
    else:  # hot terms: df ~ n_docs, negative idf, tile ranges of thousands of postings
        c = synth.zipf_corpus_np(n, 5_000, 40, seed=413)
        q = synth.queries_np(24, c.vocab, 8, seed=414, dist="zipf")
    df, idf, avgdl = synth.corpus_stats(c)
    if corpus == "zipf":
        assert df.max() > 0.9 * n and idf.min() < 0
    assert np.array_equal(c.data, c.data.astype(np.float16).astype(np.float32))  # fp16-exact stored values
    full = _full(c, idf, avgdl, q, tfidf=kind != "bm25_f32")
    if corpus == "zipf":
        assert (full < 0).any()
    rng = np.random.default_rng(415)
    layouts = [(tl, 0, keep) for tl in (9, 12, 14) for keep in (False, True)] + [(14, 4, True)]
    for tile_log2, unit_tiles, keep in layouts:
        label = f"{corpus} {kind} tile_log2={tile_log2} unit_tiles={unit_tiles} keep_canonical={keep}"
        if kind == "bm25_f32":
            ix = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, tile_log2=tile_log2,
                                         unit_tiles=unit_tiles, keep_canonical=keep)
        else:
            ix = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, mode="dot", val_dtype=kind[-3:], tile_log2=tile_log2,
                                         unit_tiles=unit_tiles, keep_canonical=keep)
        if unit_tiles == 4:
            assert ix.post16 is None and ix.post is not None, label  # units of 65 536 docs: canonical blocks only
        elif keep:
            assert ix.post16 is not None and ix.post is not None, label
        else:
            assert ix.post16 is not None and ix.post is None, label
        rows = ix.search(*q, 50)
        # the search triple as it is: count + -1 padding
        got = ix.score_docs(*q, rows[0], rows[2])
        assert_bits_equal(got, gather_expected(full, rows[0], rows[2]), label + " search rows")
        assert_bits_equal(got, rows[1], label + " search rows vs their own scores")
        G = 1 << tile_log2
        cand = _mixed_candidates(rng, rows, n, G, ix.unit_tiles * G)
        assert_bits_equal(ix.score_docs(*q, cand), gather_expected(full, cand), label + " mixed")
        count = rng.integers(-2, cand.shape[1] + 3, size=cand.shape[0]).astype(np.int32)
        assert_bits_equal(ix.score_docs(*q, cand, count), gather_expected(full, cand, count), label + " mixed + count")
        ix.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. shapes, term order, negative idf
# ---------------------------------------------------------------------------------------------------------------
def test_shapes(rx):
    from sparse_rx import synth
    n = 20_000
    c = synth.zipf_corpus_np(n, 3_000, 30, seed=421)
    _, idf, avgdl = synth.corpus_stats(c)
    lengths = ([300, 0, 65, 1, 64, 8] * 171)[:1024]
    q = _queries_of_lengths(lengths, c.vocab, seed=422)
    full = _full(c, idf, avgdl, q)
    rng = np.random.default_rng(423)
    for keep, tile_log2 in ((False, 10), (True, 14)):
        ix = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, tile_log2=tile_log2,
                                     keep_canonical=keep)
        for nq in (1, 3, 1024):
            sub = (q[0][: nq + 1], q[1][: q[0][nq]], q[2][: q[0][nq]])
            for m in (1, 7, 64, 65, 100, 1000, 4096):
                cand = rng.integers(-1, n + 1, size=(nq, m)).astype(np.int32)
                assert_bits_equal(ix.score_docs(*sub, cand), gather_expected(full[:nq], cand), f"nq={nq} m={m} keep={keep}")
        # m = n_docs: a full score vector
        cand = np.tile(np.arange(n, dtype=np.int32), (6, 1))
        sub = (q[0][:7], q[1][: q[0][6]], q[2][: q[0][6]])
        assert_bits_equal(ix.score_docs(*sub, cand), full[:6], "m = n_docs")
        ix.close()


def test_term_order_and_negative_idf(rx):
    from sparse_rx import synth
    n = 30_000
    c = synth.zipf_corpus_np(n, 2_000, 40, seed=431)
    df, idf, avgdl = synth.corpus_stats(c)
    assert idf.min() < 0
    asc = _queries_of_lengths([300, 64, 12], c.vocab, seed=432, weights="learned")
    rev_t, rev_w = asc[1].copy(), asc[2].copy()
    for i in range(3):
        lo, hi = asc[0][i], asc[0][i + 1]
        rev_t[lo:hi], rev_w[lo:hi] = asc[1][lo:hi][::-1], asc[2][lo:hi][::-1]
    rev = (asc[0], rev_t, rev_w)
    hot = np.argsort(idf)[:6].astype(np.int32)  # the six most negative idf
    neg = (np.array([0, 6], np.int32), np.sort(hot), np.ones(6, np.float32))
    full_asc, full_rev, full_neg = _full(c, idf, avgdl, asc), _full(c, idf, avgdl, rev), _full(c, idf, avgdl, neg)
    # the oracle side: the order is part of the contract, and negative scores exist
    assert not np.array_equal(full_asc.view(np.uint32), full_rev.view(np.uint32))
    assert (full_neg < 0).any() and not (full_neg > 0).any()
    cand = np.tile(np.arange(n, dtype=np.int32), (3, 1))
    for keep, tile_log2 in ((False, 9), (True, 12), (True, 14)):
        ix = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, tile_log2=tile_log2,
                                     keep_canonical=keep, unit_tiles=4 if tile_log2 == 14 else 0)
        assert_bits_equal(ix.score_docs(*asc, cand), full_asc, f"ascending terms tile_log2={tile_log2}")
        assert_bits_equal(ix.score_docs(*rev, cand), full_rev, f"reversed terms tile_log2={tile_log2}")
        got = ix.score_docs(*neg, cand[:1])
        assert_bits_equal(got, full_neg, f"negative idf tile_log2={tile_log2}")
        assert (got < 0).any()  # returned as they are: no score > 0 filter
        assert ix.search(*neg, 10)[2][0] == 0  # ... while the search returns none of them
        ix.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. doc_base
# ---------------------------------------------------------------------------------------------------------------
def test_doc_base(rx):
    from sparse_rx import synth
    n, base = 60_000, 5_000_000
    c = synth.uniform_corpus_np(n, 8_000, 30, seed=441)
    _, idf, avgdl = synth.corpus_stats(c)
    q = synth.queries_np(32, c.vocab, 8, seed=442)
    full = _full(c, idf, avgdl, q)
    rng = np.random.default_rng(443)
    local = rng.integers(0, n, size=(32, 200)).astype(np.int32)
    for keep in (False, True):
        ix0 = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, tile_log2=11, keep_canonical=keep)
        ixb = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, tile_log2=11, keep_canonical=keep,
                                      doc_base=base)
        exp = gather_expected(full, local)
        assert_bits_equal(ix0.score_docs(*q, local), exp, "doc_base 0")
        assert_bits_equal(ixb.score_docs(*q, local + base), exp, "global ids in, same bits out")
        assert not ixb.score_docs(*q, local).view(np.uint32).any()  # local ids are out of range there: +0
        edge = np.tile(np.array([base - 1, base, base + n - 1, base + n, 0, -1], np.int32), (32, 1))
        assert_bits_equal(ixb.score_docs(*q, edge), gather_expected(full, edge, doc_base=base), "doc_base edges")
        rows = ixb.search(*q, 20)
        assert rows[0][rows[0] >= 0].min() >= base
        assert_bits_equal(ixb.score_docs(*q, rows[0], rows[2]), rows[1], "doc_base: search rows")
        ix0.close()
        ixb.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. self-consistency with the search at C2 size
# ---------------------------------------------------------------------------------------------------------------
def test_c2_search_rows_score_to_their_own_bits(rx):
    import torch
    from sparse_rx import synth
    dev = torch.device("cuda:0")
    n, V = 1_000_000, 50_000
    rows_t, cols, tf, dl = synth.uniform_chunk_torch(0, n, V, 50, 20252, dev)
    df = torch.bincount(cols, minlength=V).cpu().numpy()
    idf = np.log((n - df + 0.5) / (df + 0.5)).astype(np.float32)
    avgdl = float(np.mean(dl.cpu().numpy()))
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(rows_t, minlength=n), 0)
    host = (indptr.cpu().numpy(), cols.cpu().numpy(), tf.cpu().numpy(), dl.cpu().numpy())
    q = synth.queries_np(1024, V, 8, seed=20253)
    sample = np.arange(0, 1024, 43)[:24]
    assert len(sample) == 24
    for keep in (False, True):
        ix = rx.DeviceIndex.from_coo(rows_t, cols, tf, torch.as_tensor(idf, device=dev), n, doc_lengths=dl, avgdl=avgdl, device=dev,
                                     keep_canonical=keep)
        for k in (100, 1000):  # tier 1 / tier 2
            d, s, cnt = ix.search(*q, k)
            assert cnt.min() > 0
            got = ix.score_docs(*q, d, cnt)
            assert_bits_equal(got, s, f"C2 k={k} keep_canonical={keep}")
            if k == 100:
                for qi in sample:
                    lo, hi = q[0][qi], q[0][qi + 1]
                    full = oracle.scores_given_order(*host, idf, q[1][lo:hi], q[2][lo:hi], 1.2, 0.75, avgdl)
                    assert_bits_equal(got[qi: qi + 1], gather_expected(full[None, :], d[qi: qi + 1], cnt[qi: qi + 1]), f"C2 oracle sample q={qi}")
        ix.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. streams, out= reuse, no side effect on the index
# ---------------------------------------------------------------------------------------------------------------
def test_stream_out_reuse_and_no_side_effects(rx):
    import torch
    from sparse_rx import synth
    n = 100_000
    c = synth.uniform_corpus_np(n, 10_000, 30, seed=451)
    _, idf, avgdl = synth.corpus_stats(c)
    q = synth.queries_np(300, c.vocab, 8, seed=452)
    full = _full(c, idf, avgdl, q)
    ix = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, tile_log2=12, keep_canonical=False)
    before = ix.search(*q, 100)
    dq = [torch.as_tensor(x, device="cuda:0") for x in q]
    rng = np.random.default_rng(453)
    cands = [rng.integers(-3, n + 3, size=(300, 128)).astype(np.int32) for _ in range(3)]
    out = torch.full((300, 128), float("nan"), dtype=torch.float32, device="cuda:0")
    side = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for cand in cands:  # the same `out` three times on a non-default stream, in stream order
            cd = torch.as_tensor(cand, device="cuda:0")
            r = ix.score_docs_device(*dq, cd, out=out)
            assert r is out
            got = out.cpu().numpy()  # a copy on the current (side) stream: ordered behind the kernel
            assert_bits_equal(got, gather_expected(full, cand), "side stream, out= reuse")
        cnt = torch.as_tensor(np.full(300, 5, np.int32), device="cuda:0")
        r = ix.score_docs_device(*dq, torch.as_tensor(cands[0], device="cuda:0"), cnt)
        assert_bits_equal(r.cpu().numpy(), gather_expected(full, cands[0], np.full(300, 5)), "side stream, fresh out, count")
    side.synchronize()
    for bad in (torch.empty((300, 127), dtype=torch.float32, device="cuda:0"), torch.empty((300, 128), dtype=torch.float16, device="cuda:0")):
        with pytest.raises(ValueError):
            ix.score_docs_device(*dq, torch.as_tensor(cands[0], device="cuda:0"), out=bad)
    with pytest.raises(ValueError, match="rows"):
        ix.score_docs(*q, cands[0][:10])
    after = ix.search(*q, 100)
    for a, b_ in zip(before, after):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b_.view(np.uint32) if b_.dtype == np.float32 else b_)
    # the descriptor follows the handle: new bounds, then the dropped canonical copy
    ix2 = rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, tile_log2=12)
    exp = gather_expected(full, cands[1])
    assert_bits_equal(ix2.score_docs(*q, cands[1]), exp, "both copies")
    ix2.set_term_bound(None)
    assert_bits_equal(ix2.score_docs(*q, cands[1]), exp, "after set_term_bound")
    assert ix2.drop_canonical() and ix2.post is None
    assert_bits_equal(ix2.score_docs(*q, cands[1]), exp, "after drop_canonical")
    assert ix.score_docs(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros((0, 4), np.int32)).shape == (0, 4)
    ix.close()
    ix2.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the sharded path on one GPU (RCCL group of one rank)
# ---------------------------------------------------------------------------------------------------------------
def test_sharded_service_on_one_gpu(rx, golden_dir):
    import socket
    import torch
    import torch.distributed as dist
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        z = np.load(os.path.join(golden_dir, "text_small.npz"))
        with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
            j = json.load(f)
        doc_ids = [str(d) for d in z["doc_ids"]]
        qids = [str(q) for q in z["score_qids"]]
        svc = rx.RetrievalService(device="cuda:0", tile_log2=6, sharded=True)
        svc.build_bm25_index(j["corpus"])
        assert svc._be.searcher is not None and svc._be.searcher.local_score is not None and svc._be.searcher.force_exchange
        got = svc.score_bm25({q: j["queries"][q] for q in qids}, {q: doc_ids for q in qids})
        assert_bits_equal(_rows(got, qids, doc_ids), z["full_scores"], "sharded service, one rank")
        svc._be.searcher.close()
        svc.close()
    finally:
        dist.destroy_process_group()
