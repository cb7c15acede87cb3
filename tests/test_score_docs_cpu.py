"""srx_score_docs without a GPU: the layout walk restated in NumPy against the reference-written score vectors, the C
ABI's argument checks (none reaches a device), the host-side candidate validation, and the sharded protocol + the API
mirrors under gloo with the CPU oracle behind ``local_score``."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from oracle import np_oracle
from parity import np_build_blocks, np_compact_blocks
from score_ref import assert_bits_equal, gather_expected, np_score_docs, oracle_full_scores


# ---------------------------------------------------------------------------------------------------------------
# 1. the walk over the blocked layout reproduces the reference's own score vectors
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_log2,unit_tiles", [(9, 2), (8, 3), (12, 1)])
@pytest.mark.parametrize("mode", ["tfidf", "bm25"])
def test_layout_walk_reproduces_reference_vectors(golden_dir, mode, tile_log2, unit_tiles):
    """np_score_docs on the canonical blocks and on the compact copy == csr_zipf.npz:tfidf_full / bm25_full, bit for bit,
    on all 3 000 docs of the 16 queries."""
    z = np.load(os.path.join(golden_dir, "csr_zipf.npz"))
    n_docs, vocab = (int(x) for x in z["tf_shape"])
    indptr, indices = z["tf_indptr"], z["tf_indices"]
    if mode == "bm25":
        rows = np.repeat(np.arange(n_docs), np.diff(indptr))
        data = np_oracle.impacts_f32(z["tf_data"], rows, z["doc_lengths"], float(z["k1"]), float(z["b"]), float(z["avgdl"]))
        idf, exp = z["idf"], z["bm25_full"]
    else:
        data, idf, exp = z["tf_data"], z["idf_tfidf"], z["tfidf_full"]
    nq = exp.shape[0]
    assert exp.shape == (16, 3000)
    term_ptr, post, skip, _ = np_build_blocks(indptr, indices, data, n_docs, vocab, tile_log2, unit_tiles)
    q_ptr = z["q_ptr"][: nq + 1]
    cand = np.tile(np.arange(n_docs, dtype=np.int32), (nq, 1))
    got = np_score_docs(term_ptr, post, skip, idf, n_docs, tile_log2, unit_tiles, q_ptr, z["q_term"], z["q_weight"], cand)
    assert_bits_equal(got, exp, f"canonical {mode} ({tile_log2}, {unit_tiles})")
    post16 = np_compact_blocks(post, unit_tiles << tile_log2)
    got = np_score_docs(term_ptr, post16, skip, idf, n_docs, tile_log2, unit_tiles, q_ptr, z["q_term"], z["q_weight"], cand, compact=True)
    assert_bits_equal(got, exp, f"compact {mode} ({tile_log2}, {unit_tiles})")


def test_layout_walk_padding_range_and_doc_base(golden_dir):
    """The output contract of the restatement itself: padding and ids outside the shard give +0, global ids are rebased."""
    z = np.load(os.path.join(golden_dir, "csr_zipf.npz"))
    n_docs, vocab = (int(x) for x in z["tf_shape"])
    term_ptr, post, skip, _ = np_build_blocks(z["tf_indptr"], z["tf_indices"], z["tf_data"], n_docs, vocab, 9, 2)
    base = 5_000_000
    cand = np.array([[base + 7, base + 2999, 7, -1, base + 3000, base - 1, base + 7, 2 ** 31 - 1]] * 2, np.int32)
    count = np.array([8, 2], np.int32)
    got = np_score_docs(term_ptr, post, skip, z["idf_tfidf"], n_docs, 9, 2, z["q_ptr"][:3], z["q_term"], z["q_weight"], cand, count,
                        doc_base=base)
    exp = gather_expected(z["tfidf_full"][:2], cand, count, doc_base=base)
    assert_bits_equal(got, exp, "doc_base")
    assert got[0, 0] == z["tfidf_full"][0, 7] and got[0, 6] == got[0, 0] and not got[0, [2, 3, 4, 5, 7]].any() and not got[1, 2:].any()


# ---------------------------------------------------------------------------------------------------------------
# 2. argument checks of the C ABI
# ---------------------------------------------------------------------------------------------------------------
def _desc(**kw):
    from sparse_rx import _capi
    d = dict(device=0, val_type=0, n_docs=100_000, vocab=50, nnz=1000, n_blocks=300, doc_base=0, tile_log2=12, n_tiles=25,
             unit_tiles=3, reserved0=0, term_ptr=1 << 20, post=1 << 21, tile_skip=1 << 22, idf=1 << 23, term_bound=0, post16=1 << 24)
    d.update(kw)
    return _capi.IndexDesc(**d)


_P = (1 << 25, 1 << 26, 1 << 27, 4, 1 << 28, 1 << 29, 10, 1 << 30, None)  # q_ptr, q_term, q_weight, nq, cand_doc, cand_count, m, out, stream


def _call(desc, args=_P):
    from sparse_rx import _capi
    L = _capi.lib()
    rc = L.srx_score_docs(None if desc is None else ctypes.byref(desc), *args)
    return rc, (L.srx_last_error() or b"")


def _args(**kw):
    names = ("q_ptr", "q_term", "q_weight", "nq", "cand_doc", "cand_count", "m", "out", "stream")
    a = dict(zip(names, _P))
    a.update(kw)
    return tuple(a[n] for n in names)


@pytest.mark.parametrize("label,desc,args,word", [
    ("null descriptor", None, _P, b"null descriptor"),
    ("bad val_type", dict(val_type=7), _P, b"val_type"),
    ("n_docs 0", dict(n_docs=0, n_tiles=0), _P, b"n_docs"),
    ("vocab 0", dict(vocab=0), _P, b"vocab"),
    ("tile_log2 low", dict(tile_log2=5, n_tiles=3125), _P, b"tile_log2"),
    ("tile_log2 high", dict(tile_log2=15, n_tiles=4), _P, b"tile_log2"),
    ("n_tiles inconsistent", dict(n_tiles=24), _P, b"n_tiles"),
    ("unit_tiles 0", dict(unit_tiles=0), _P, b"unit_tiles"),
    ("unit_tiles 65", dict(unit_tiles=65), _P, b"unit_tiles"),
    ("no postings", dict(post=0, post16=0), _P, b"neither post nor post16"),
    ("post16 with a wide unit", dict(tile_log2=14, n_tiles=7, unit_tiles=4), _P, b"49152"),
    ("null term_ptr", dict(term_ptr=0), _P, b"term_ptr"),
    ("null tile_skip", dict(tile_skip=0), _P, b"tile_skip"),
    ("null idf", dict(idf=0), _P, b"idf"),
    ("nq < 0", {}, _args(nq=-1), b"nq < 0"),
    ("m < 1", {}, _args(m=0), b"m must be"),
    ("nq * m overflow", {}, _args(nq=1 << 16, m=1 << 15), b"nq * m"),
    ("null q_ptr", {}, _args(q_ptr=None), b"null q_ptr"),
    ("null cand_doc", {}, _args(cand_doc=None), b"null q_ptr"),
    ("null out_score", {}, _args(out=None), b"null q_ptr"),
])
def test_score_docs_refusals(label, desc, args, word):
    """Every refusal of the header returns SRX_ERR_INVALID with the function's name in srx_last_error(), before anything
    touches a device (the pointers are fakes: a launch would fault, a device call would fail differently on a CPU box)."""
    rc, msg = _call(None if desc is None else _desc(**desc), args)
    assert rc == -1, (label, rc, msg)
    assert msg.startswith(b"srx_score_docs:") and word in msg, (label, msg)


def test_score_docs_nq_zero_is_ok_without_a_launch():
    assert _call(_desc(), _args(nq=0, q_ptr=None, cand_doc=None, out=None))[0] == 0
    assert _call(_desc(post16=0), _args(nq=0))[0] == 0            # canonical only
    assert _call(_desc(post=0, val_type=1), _args(nq=0))[0] == 0  # compact only, fp16 values
    # a unit of more than 49 152 docs is fine without a compact copy
    assert _call(_desc(tile_log2=14, n_tiles=7, unit_tiles=4, post16=0), _args(nq=0))[0] == 0
    # (nq * m == 2^31 - 1 is the largest block)
    assert _call(_desc(), _args(nq=0, m=2 ** 31 - 1))[0] == 0


def test_symbol_is_declared_bound_and_listed():
    from sparse_rx import _capi
    assert "srx_score_docs" in _capi.SYMBOLS and "score_docs.hip" in _capi.SOURCES and len(_capi.SYMBOLS) == 35
    assert _capi.lib().srx_version() == 301
    assert _capi.kernel_sources_sha256() == "5b0819c0690ad23ca713f08faa3b931da0e4d43dc3e56784f282166e1203c030"


# ---------------------------------------------------------------------------------------------------------------
# 3. host-side candidate validation
# ---------------------------------------------------------------------------------------------------------------
def test_validate_candidates():
    from sparse_rx.index import validate_candidates
    d, c = validate_candidates([[1, 2, -1], [5, 2 ** 31 - 1, -7]], None, 2)
    assert d.dtype == np.int32 and d.shape == (2, 3) and d.flags.c_contiguous and c is None
    d, c = validate_candidates(np.array([[1, 2]], np.int64), np.array([-3], np.int64), 1)
    assert d.dtype == np.int32 and c.dtype == np.int32 and c.tolist() == [-3]
    d, c = validate_candidates(np.zeros((0, 4), np.int32), np.zeros(0, np.int32), 0)
    assert d.shape == (0, 4)
    for cand, count, nq, msg in (([1, 2, 3], None, 3, "2-D"), ([[1.0, 2.0]], None, 1, "integer"), ([[1, 2]], None, 2, "rows"),
                                 (np.zeros((2, 0), np.int32), None, 2, "m >= 1"), ([[2 ** 31]], None, 1, "int32"),
                                 ([[-2 ** 31 - 1]], None, 1, "int32"), ([[1, 2]], [1, 2], 1, "length 1"),
                                 ([[1, 2]], [[1]], 1, "1-D"), ([[1, 2]], [1.5], 1, "integer"), ([[1, 2]], [2 ** 40], 1, "int32")):
        with pytest.raises(ValueError, match=msg):
            validate_candidates(cand, count, nq)


# ---------------------------------------------------------------------------------------------------------------
# 5. without a GPU
# ---------------------------------------------------------------------------------------------------------------
def test_score_before_build_raises_like_search():
    import sparse_rx
    svc = sparse_rx.RetrievalService()
    with pytest.raises(ValueError, match="BM25 index not built"):
        svc.score_bm25({"a": "b"}, {"a": ["d"]})
    for r in (sparse_rx.OptimizedBM25Retriever(), sparse_rx.OptimizedRetriever({"type": "bm25"})):
        with pytest.raises(ValueError, match="Index not built"):
            r.score({"a": "b"}, {"a": ["d"]})
    s = sparse_rx.ShardedSearcher(None, None, None)  # the existing positional form: no local_score
    with pytest.raises(ValueError, match="local_score"):
        s.score_docs(None, None, None, None)


# ---------------------------------------------------------------------------------------------------------------
# 4. the sharded protocol and the API mirrors under gloo
# ---------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _scoring_searcher_factory(host, doc_base, mode, k1, b, group):
    """TEST backend: the CPU oracle scores this rank's rows -- ``oracle.scores_given_order`` behind ``local_score``, the
    oracle search of test_distributed_cpu behind ``local_search`` (the product wiring puts the HIP engine at both)."""
    import sparse_rx
    from test_distributed_cpu import _merge_packed, _oracle_searcher_factory, _pack
    base = _oracle_searcher_factory(host, doc_base, mode, k1, b, group)

    def local_score(q_ptr, q_term, q_w, cand_doc, cand_count=None):
        full = oracle_full_scores(oracle, host.indptr, host.indices, host.data, host.doc_lengths, host.idf, q_ptr.numpy(), q_term.numpy(),
                                  q_w.numpy(), k1, b, host.avgdl, tfidf=(mode != "bm25"))
        return torch.from_numpy(gather_expected(full, cand_doc.numpy(), None if cand_count is None else cand_count.numpy(), doc_base))

    return sparse_rx.ShardedSearcher(base.local_search, _pack, _merge_packed, group, local_score=local_score)


def _as_rows(got, qids, doc_ids):
    return np.array([[got[q][d] for d in doc_ids] for q in qids], np.float32)


def _score_worker(rank, world, port, golden_dir, tmp, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sparse_rx
    z = np.load(os.path.join(golden_dir, "text_small.npz"))
    p = np.load(os.path.join(golden_dir, "pipeline_small.npz"))
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        j = json.load(f)
    doc_ids = [str(d) for d in z["doc_ids"]]
    qids = [str(q) for q in z["score_qids"]]
    svc = sparse_rx.RetrievalService(shard_searcher_factory=_scoring_searcher_factory)
    svc.build_bm25_index(j["corpus"])
    queries = {q: j["queries"][q] for q in qids}
    got = svc.score_bm25(queries, {q: doc_ids for q in qids})
    assert list(got) == qids and all(list(got[q]) == doc_ids for q in qids)  # every candidate, the caller's order
    assert_bits_equal(_as_rows(got, qids, doc_ids), z["full_scores"], f"rank {rank}: score_bm25 vs full_scores")
    # ragged lists, a qid without candidates, a blank and an all-OOV query, an unknown id
    full = {q: z["full_scores"][i] for i, q in enumerate(qids)}
    row = {d: i for i, d in enumerate(doc_ids)}
    q0, q1, q2 = qids[0], qids[1], qids[2]
    lists = {q0: doc_ids[5:6], q1: doc_ids[::-7], q2: [], "blank": doc_ids[:3], "oov": doc_ids[100:104]}
    rag = svc.score_bm25({q0: queries[q0], q1: queries[q1], q2: queries[q2], "blank": "   ", "oov": "zzzunknown qqqmissing", "none": queries[q0]}, lists)
    assert list(rag) == [q0, q1, q2, "blank", "oov", "none"]
    assert rag[q2] == {} and rag["none"] == {}
    assert rag["blank"] == {d: 0.0 for d in doc_ids[:3]} and rag["oov"] == {d: 0.0 for d in doc_ids[100:104]}
    for q in (q0, q1):
        assert list(rag[q]) == lists[q]
        assert_bits_equal(np.array(list(rag[q].values()), np.float32), full[q][[row[d] for d in lists[q]]], f"rank {rank}: ragged {q}")
    with pytest.raises(ValueError, match="no-such-doc"):
        svc.score_bm25({q0: queries[q0]}, {q0: [doc_ids[0], "no-such-doc"]})
    # k1 / b are plain attributes: the scores follow them like search_bm25's
    svc.k1 = 1.6
    moved = svc.score_bm25({q0: queries[q0]}, {q0: doc_ids})
    h = svc.host
    a, b_ = sparse_rx.shard_range(len(doc_ids), world, rank)
    qp, qt, qw = sparse_rx.encode_queries([queries[q0]], h.vocabulary)
    exp_local = oracle.scores_given_order(h.indptr, h.indices, h.data, h.doc_lengths, h.idf, qt, qw, 1.6, 0.75, h.avgdl)
    assert_bits_equal(np.array(list(moved[q0].values()), np.float32)[a:b_], exp_local, f"rank {rank}: k1 change")
    assert not np.array_equal(np.array(list(moved[q0].values()), np.float32), full[q0])
    svc.close()
    # the pipeline twin in query-token order, and the registry twin
    pq = [str(q) for q in p["bm25_qids"]]
    ret_ = sparse_rx.OptimizedRetriever({"type": "bm25"}, accumulation="token", cache_dir=tmp, shard_searcher_factory=_scoring_searcher_factory)
    ret_.build_index_from_corpus(j["corpus"])
    got = ret_.score({q: j["queries"][q] for q in pq}, {q: doc_ids for q in pq})
    assert_bits_equal(_as_rows(got, pq, doc_ids), p["bm25_full_scores"], f"rank {rank}: OptimizedRetriever token order")
    ret_.close()
    sp = sparse_rx.OptimizedRetriever({"type": "splade"}, accumulation="token", cache_dir=tmp, shard_searcher_factory=_scoring_searcher_factory)
    sp.build_index_from_corpus(j["corpus"])
    sq = [str(q) for q in p["splade_qids"]]
    got = sp.score({q: j["queries"][q] for q in sq}, {q: doc_ids for q in sq})
    assert_bits_equal(_as_rows(got, sq, doc_ids), p["splade_full_scores"], f"rank {rank}: OptimizedRetriever splade")
    sp.close()
    reg = sparse_rx.OptimizedBM25Retriever(shard_searcher_factory=_scoring_searcher_factory)
    reg.build_index_from_corpus(j["corpus"])
    got = reg.score(queries, {q: doc_ids for q in qids})
    assert_bits_equal(_as_rows(got, qids, doc_ids), z["full_scores"], f"rank {rank}: OptimizedBM25Retriever")
    reg.close()
    ret[rank] = True
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_score_apis_shard_under_torch_distributed(world, golden_dir, tmp_path):
    """RetrievalService.score_bm25 / OptimizedRetriever.score / OptimizedBM25Retriever.score called by every rank of a gloo
    group: every rank scores the whole candidate block on its doc range, one all-reduce sums the blocks, and every rank
    returns the reference's own full score vectors (text_small.npz:full_scores, pipeline_small.npz:*_full_scores) bit
    for bit."""
    ctx = mp.get_context("spawn")
    with ctx.Manager() as m:
        ret = m.dict()
        port = _free_port()
        procs = [ctx.Process(target=_score_worker, args=(r, world, port, golden_dir, str(tmp_path), ret)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        assert dict(ret) == {r: True for r in range(world)}
