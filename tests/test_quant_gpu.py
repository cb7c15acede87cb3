"""The device quantisers on the GPU (include/sparse_rx_quant.h, csrc/dense_quant.hip): every comparison is on code bytes and
fp32 bits against the NumPy restatement tests/quant_ref.py, which tests/test_quant_cpu.py pins to the host quantisers and to
the reference-written fixtures.  Then the doors: ``from_embeddings`` and ``quantize="device"`` give the tensors and the dicts of
the host route exactly."""
import functools
import json
import os

import numpy as np
import pytest

import quant_ref
import sparse_rx
from quant_ref import same_bits
from sparse_rx import _capi, dense

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 31, 32, 33, 48, 63, 64, 65, 100, 768, 1000, 1024)
NROWS = (1, 31, 32, 33, 300, 1000)
JUNK = 0x55


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _views(e):
    """The same rows as the kernels can meet them: (name, device view).  ``dense``: ld == dim (16-byte loads when dim % 4 == 0);
    ``slice``: a column slice of a tensor 3 columns wider, one column in (4-byte aligned base, unaligned rows: 4-byte loads);
    ``wide``: dim % 4 == 0 only, ld = dim + 4 (16-byte loads with a row stride)."""
    torch = _torch()
    n, dim = e.shape
    out = [("dense", _dev(e))]
    w = torch.full((n, dim + 3), float("nan"), dtype=torch.float32, device="cuda:0")
    w[:, 1: dim + 1] = _dev(e)
    out.append(("slice", w[:, 1: dim + 1]))
    if dim % 4 == 0:
        w4 = torch.full((n, dim + 4), float("nan"), dtype=torch.float32, device="cuda:0")
        w4[:, :dim] = _dev(e)
        out.append(("wide", w4[:, :dim]))
    return out


def _junk(shape, dtype):
    torch = _torch()
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), dtype=dtype, device="cuda:0")
    return torch.full(shape, JUNK, dtype=dtype, device="cuda:0")


def _run(entry, x, dim_pad, outs, flag=None, row0=0, n_total=None, packed=None):
    """One launch through the package's own launcher; the outputs and the flag word as host arrays."""
    flag = dense._quantize_device(entry, x, dim_pad, outs, flag, row0, n_total, packed)
    _torch().cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in outs], int(flag.item())


def _i8_rows(x, n, dim_pad, packed=0, **kw):
    torch = _torch()
    nbytes = _capi.lib().srx_dense_packed_bytes(n, dim_pad) if packed else n * dim_pad
    outs = (_junk((nbytes,), torch.int8), _junk((n,), torch.float32))
    (codes, scales), flag = _run("srx_dense_quantize_i8", x, dim_pad, outs, n_total=n, packed=packed, **kw)
    return (codes if packed else codes.reshape(n, dim_pad)), scales, flag


def _u8_rows(x, n, dim_pad):
    torch = _torch()
    outs = (_junk((n, dim_pad), torch.uint8), _junk((2 * n,), torch.float32))
    (codes, table), flag = _run("srx_dense_quantize_u8", x, dim_pad, outs, n_total=n)
    return codes, table, flag


def _i8_queries(x, n, dim_pad):
    torch = _torch()
    outs = (_junk((n, dim_pad), torch.int8), _junk((n,), torch.float32))
    (codes, scales), flag = _run("srx_dense_quantize_queries_i8", x, dim_pad, outs)
    return codes, scales, flag


def _u8_queries(x, n, dim_pad, codes=True):
    torch = _torch()
    outs = (_junk((n, dim_pad), torch.uint8) if codes else None, _junk((n, 2), torch.float32) if codes else None,
            _junk((n, dim_pad), torch.float32))
    (u8, pairs, deq), flag = _run("srx_dense_quantize_queries_u8", x, dim_pad, outs)
    return u8, pairs, deq, flag


def _assert_same(got, exp, what):
    for g, e in zip(got, exp):
        if isinstance(e, int):
            assert g == e, (what, "flag", g, e)
        else:
            assert same_bits(g, e), (what, np.argwhere(np.ascontiguousarray(g).view(np.uint8).reshape(-1) !=
                                                       np.ascontiguousarray(e).view(np.uint8).reshape(-1))[:4].tolist())


@functools.lru_cache(maxsize=None)
def _case(dim, n):
    """Rows and query rows of one shape with their restated results, computed once and left unchanged."""
    rows = quant_ref.make_rows(1000 * dim + n, n, dim)
    qrows = quant_ref.make_rows(7 + 1000 * dim + n, n, dim, degenerate=False, denormal=False)
    if dim == 1:  # a 1-d query is constant: degenerate in the asymmetric scheme, which test_flags covers
        uq = None
    else:
        uq = quant_ref.u8_queries(qrows, quant_ref.pad_u8(dim))
    return (rows, qrows, quant_ref.i8_rows(rows, quant_ref.pad_i8(dim)), quant_ref.u8_rows(rows, quant_ref.pad_u8(dim)),
            quant_ref.i8_queries(qrows, quant_ref.pad_i8(dim)), uq)


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    z = np.load(os.path.join(golden_dir, "dense_int8.npz"))
    a = np.load(os.path.join(golden_dir, "dense_uint8_asym.npz"))
    j = json.load(open(os.path.join(golden_dir, "dense_int8.json")))
    return z, a, j


def test_both_fixtures_corpus_and_queries(fixtures):
    z, a, _ = fixtures
    emb, qemb = _dev(z["emb"]), _dev(z["qemb"])
    c, s, flag = sparse_rx.quantize_symmetric_device(emb)
    assert tuple(c.shape) == (300, 48) and c._base.shape[1] == 64 and not c._base[:, 48:].any()
    assert flag.item() == 0 and same_bits(c.cpu().numpy(), z["corpus_int8"]) and same_bits(s.cpu().numpy(), z["corpus_scales"])
    c, s, flag = sparse_rx.quantize_queries_symmetric_device(qemb)
    assert flag.item() == 0 and same_bits(c.cpu().numpy(), z["query_int8"]) and same_bits(s.cpu().numpy(), z["query_scales"])
    c, s, flag = sparse_rx.quantize_asymmetric_device(emb)
    assert flag.item() == 0 and same_bits(c.cpu().numpy(), a["corpus_uint8"]) and same_bits(s.cpu().numpy(), a["corpus_scales"])
    c, s, deq, flag = sparse_rx.quantize_queries_asymmetric_device(qemb)
    assert flag.item() == 0 and same_bits(c.cpu().numpy(), a["query_uint8"]) and same_bits(s.cpu().numpy(), a["query_scales"])
    exp = np.stack([dense.dequantize_query_asymmetric(q, p) for q, p in zip(a["query_uint8"], a["query_scales"])])
    assert same_bits(deq.cpu().numpy(), exp) and not deq._base[:, 48:].any()
    none_c, none_s, deq2, _ = sparse_rx.quantize_queries_asymmetric_device(qemb, codes=False)
    assert none_c is None and none_s is None and same_bits(deq2.cpu().numpy(), exp)


@pytest.mark.parametrize("dim", DIMS)
def test_bits_at_every_row_count_and_stride(dim):
    pi, pu = quant_ref.pad_i8(dim), quant_ref.pad_u8(dim)
    for n in NROWS:
        rows, qrows, ri, ru, qi, qu = _case(dim, n)
        assert ri[2] == 0 and ru[2] == 0 and qi[2] == 0 and (qu is None or qu[3] == 0)
        for name, x in _views(rows):
            _assert_same(_i8_rows(x, n, pi), ri, ("i8 rows", dim, n, name))
            _assert_same(_u8_rows(x, n, pu), ru, ("u8 rows", dim, n, name))
        for name, x in _views(qrows):
            _assert_same(_i8_queries(x, n, pi), qi, ("i8 queries", dim, n, name))
            if qu is not None:
                _assert_same(_u8_queries(x, n, pu), qu, ("u8 queries", dim, n, name))
    if dim in (3, 768):  # only the de-quantised block wanted: the two NULL outputs
        rows, qrows, *_, qu = _case(dim, 33)
        got = _u8_queries(_dev(qrows), 33, pu, codes=False)
        assert got[0] is None and got[1] is None and same_bits(got[2], qu[2]) and got[3] == 0


@pytest.mark.parametrize("dim", (31, 100, 768, 1000))
def test_packed_output_is_the_pack_of_the_row_major_output(dim):
    torch = _torch()
    L = _capi.lib()
    dim_pad = quant_ref.pad_i8(dim)
    for n in (1, 32, 33, 300):
        rows, _, ri, *_ = _case(dim, n)
        x = _dev(rows)
        packed, scales, flag = _i8_rows(x, n, dim_pad, packed=1)
        assert flag == 0 and same_bits(scales, ri[1])
        exp = _junk((L.srx_dense_packed_bytes(n, dim_pad),), torch.int8)
        rm = _dev(ri[0])  # == the kernel's own row-major output (test_bits_at_every_row_count_and_stride)
        _capi.check(L.srx_dense_pack_i8(0, rm.data_ptr(), n, dim_pad, exp.data_ptr(), None), "srx_dense_pack_i8")
        torch.cuda.synchronize()
        assert np.array_equal(packed, exp.cpu().numpy()), (dim, n)  # byte for byte, the zero rows of the last tile included
        assert np.array_equal(dense.unpack_i8_host(packed, n, dim_pad), ri[0])


@pytest.mark.parametrize("dim,chunk", [(48, 32), (100, 64), (768, 96)])
def test_chunked_builds_equal_the_one_call_build(dim, chunk):
    """row0 = 0, chunk, 2 chunk, ...; the last chunk ends inside a tile (300 = 9 * 32 + 12)."""
    torch = _torch()
    n = 300
    rows, _, ri, ru, *_ = _case(dim, n)
    pi, pu = quant_ref.pad_i8(dim), quant_ref.pad_u8(dim)
    one_packed = _i8_rows(_dev(rows), n, pi, packed=1)[0]
    for packed in (0, 1):
        nbytes = _capi.lib().srx_dense_packed_bytes(n, pi) if packed else n * pi
        outs = (_junk((nbytes,), torch.int8), _junk((n,), torch.float32))
        flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        for lo in range(0, n, chunk):
            x = _dev(rows[lo: lo + chunk])
            dense._quantize_device("srx_dense_quantize_i8", x, pi, outs, flag, lo, n, packed)
        torch.cuda.synchronize()
        codes, scales = outs[0].cpu().numpy(), outs[1].cpu().numpy()
        assert flag.item() == 0 and same_bits(scales, ri[1])
        assert np.array_equal(codes, one_packed) if packed else same_bits(codes.reshape(n, pi), ri[0])
    outs = (_junk((n, pu), torch.uint8), _junk((2 * n,), torch.float32))
    for lo in range(0, n, chunk):
        dense._quantize_device("srx_dense_quantize_u8", _dev(rows[lo: lo + chunk]), pu, outs, None, lo, n)
    torch.cuda.synchronize()
    assert same_bits(outs[0].cpu().numpy(), ru[0]) and same_bits(outs[1].cpu().numpy(), ru[1])
    # a chunk in the middle of the corpus leaves every other row alone
    outs = (_junk((n, pu), torch.uint8), _junk((2 * n,), torch.float32))
    dense._quantize_device("srx_dense_quantize_u8", _dev(rows[37: 37 + 50]), pu, outs, None, 37, n)
    torch.cuda.synchronize()
    got, table = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert same_bits(got[37:87], ru[0][37:87]) and np.all(got[:37] == JUNK) and np.all(got[87:] == JUNK)
    assert same_bits(table[37:87], ru[1][37:87]) and same_bits(table[n + 37: n + 87], ru[1][n + 37: n + 87])
    assert np.isnan(table[:37]).all() and np.isnan(table[87:n + 37]).all() and np.isnan(table[n + 87:]).all()


@pytest.mark.parametrize("dim", (3, 48, 768, 1000))
def test_flag_bits_and_defined_outputs(dim):
    torch = _torch()
    rng = np.random.default_rng(dim)
    n = 70
    e = quant_ref.make_rows(dim, n, dim, degenerate=False, denormal=False)
    assert quant_ref.i8_queries(e)[2] == 0 and quant_ref.u8_queries(e)[3] == 0
    pi, pu = quant_ref.pad_i8(dim), quant_ref.pad_u8(dim)
    for kind in ("nan", "inf", "-inf", "overflow", "zero", "constant", "mixed"):
        x = e.copy()
        where = (5, 40, 69) if kind != "mixed" else (5,)
        for r in where:
            c = int(rng.integers(0, dim))
            if kind in ("nan", "mixed"):
                x[r, c] = np.nan
            elif kind in ("inf", "-inf"):
                x[r, c] = float(kind)
            elif kind == "overflow":  # finite values whose max - min is not: flagged in the asymmetric scheme only
                x[r] = 0
                x[r, 0], x[r, -1] = 3e38, -3e38
            elif kind == "zero":
                x[r] = 0
            else:
                x[r] = -2.5
        if kind == "mixed":
            x[33] = 0
            x[66] = 1e-3
        exp = (quant_ref.i8_rows(x, pi), quant_ref.u8_rows(x, pu), quant_ref.i8_queries(x, pi), quant_ref.u8_queries(x, pu))
        bad = {"nan": 1, "inf": 1, "-inf": 1, "overflow": 0, "zero": 0, "constant": 0, "mixed": 1}[kind]
        deg = 2 if kind in ("zero", "constant", "mixed") else 0
        assert exp[0][2] == bad and exp[2][2] == bad | (deg if kind != "constant" else 0)  # a constant i8 query is an ordinary one
        assert exp[1][2] == (1 if kind == "overflow" else bad) and exp[3][3] == (1 if kind == "overflow" else bad) | deg
        d = _dev(x)
        _assert_same(_i8_rows(d, n, pi), exp[0], ("i8 rows", kind))
        _assert_same(_u8_rows(d, n, pu), exp[1], ("u8 rows", kind))
        _assert_same(_i8_queries(d, n, pi), exp[2], ("i8 queries", kind))
        _assert_same(_u8_queries(d, n, pu), exp[3], ("u8 queries", kind))
    # the bits are ORed into the word: what the caller left there stays, and a batch without a flagged row writes nothing
    for start, rows, want in ((4, e, 4), (4, x, 4 | 3), (0, e, 0)):
        flag = torch.full((1,), start, dtype=torch.int32, device="cuda:0")
        outs = (_junk((n, pi), torch.int8), _junk((n,), torch.float32))
        assert _run("srx_dense_quantize_queries_i8", _dev(rows), pi, outs, flag)[1] == want
    outs = (_junk((n, pi), torch.int8), _junk((n,), torch.float32))
    x_dev = _dev(x)
    rc = _capi.lib().srx_dense_quantize_queries_i8(0, x_dev.data_ptr(), dim, n, dim, pi, outs[0].data_ptr(), outs[1].data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc == 0 and same_bits(outs[0].cpu().numpy(), exp[2][0])  # flag == NULL: the defined outputs without the word


def test_side_stream():
    torch = _torch()
    rows, qrows, ri, ru, qi, qu = _case(768, 300)
    side = torch.cuda.Stream()
    x, q = _dev(rows), _dev(qrows)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.zeros(1 << 24, device="cuda:0").cumsum(0)  # work in front on the same stream
        x2 = torch.empty_like(x).copy_(x)
        got = (sparse_rx.quantize_symmetric_device(x2), sparse_rx.quantize_asymmetric_device(x2), sparse_rx.quantize_queries_symmetric_device(q),
               sparse_rx.quantize_queries_asymmetric_device(q))
    side.synchronize()
    host = [[t.cpu().numpy() for t in g] for g in got]
    assert same_bits(host[0][0], ri[0]) and same_bits(host[0][1], ri[1]) and host[0][2][0] == 0
    assert same_bits(host[1][0], ru[0]) and same_bits(host[1][1], ru[1])
    assert same_bits(host[2][0], qi[0]) and same_bits(host[2][1], qi[1])
    assert same_bits(host[3][0], qu[0]) and same_bits(host[3][1], qu[1]) and same_bits(host[3][2], qu[2])


@pytest.mark.parametrize("dim,n", [(48, 300), (768, 1000), (100, 33)])
def test_from_embeddings_is_the_index_of_the_host_quantisers(dim, n):
    torch = _torch()
    rows = _case(dim, n)[0]
    hc, hs = sparse_rx.quantize_symmetric(rows)
    for packed in (True, False):
        ref = sparse_rx.DenseInt8Index(hc, hs, packed=packed)
        for emb, kw in ((rows, dict(chunk_rows=64)), (rows, {}), (_dev(rows), {})):
            ix = sparse_rx.DenseInt8Index.from_embeddings(emb, packed=packed, doc_base=7, **kw)
            assert torch.equal(ix.corpus, ref.corpus) and torch.equal(ix.scales, ref.scales)
            assert (ix.n_docs, ix.dim, ix.dim_pad, ix.packed, ix.doc_base) == (n, dim, ref.dim_pad, packed, 7)
        back = ix.corpus_to_host()
        assert same_bits(back[0], hc) and same_bits(back[1], hs)
    uc, ut = sparse_rx.quantize_asymmetric(rows)
    ref = sparse_rx.DenseUint8Index(uc, ut)
    for emb, kw in ((rows, dict(chunk_rows=32)), (_dev(rows), {})):
        ix = sparse_rx.DenseUint8Index.from_embeddings(emb, **kw)
        assert torch.equal(ix.corpus, ref.corpus) and torch.equal(ix.scales, ref.scales) and (ix.dim, ix.dim_pad) == (dim, ref.dim_pad)
    back = ix.corpus_to_host()
    assert same_bits(back[0], uc) and same_bits(back[1], ut)


def test_from_embeddings_refusals():
    rows = _case(48, 300)[0].copy()
    for cls in (sparse_rx.DenseInt8Index, sparse_rx.DenseUint8Index):
        for bad in (48, 0, -32, 31):
            with pytest.raises(ValueError, match="multiple of 32"):
                cls.from_embeddings(rows, chunk_rows=bad)
        with pytest.raises(ValueError, match="Empty corpus"):
            cls.from_embeddings(rows[:0])
    rows[123, 7] = np.nan
    for cls in (sparse_rx.DenseInt8Index, sparse_rx.DenseUint8Index):
        for emb in (rows, _dev(rows)):
            with pytest.raises(ValueError, match="non-finite"):
                cls.from_embeddings(emb, chunk_rows=64)
    with pytest.raises(ValueError, match="1024"):
        sparse_rx.DenseInt8Index.from_embeddings(np.zeros((4, 1025), np.float32))


def _triples_equal(a, b):
    torch = _torch()
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_f32_query_doors_of_the_indexes():
    torch = _torch()
    rows, qrows = _case(100, 1000)[0], _case(100, 300)[1][:40]
    ix = sparse_rx.DenseInt8Index.from_embeddings(rows)
    qq = [sparse_rx.quantize_query_symmetric(q) for q in qrows]
    qi, qs = _dev(np.stack([a for a, _ in qq])), _dev(np.array([b for _, b in qq], np.float32))
    cand = torch.as_tensor(np.random.default_rng(0).integers(0, 1000, (40, 17)).astype(np.int32), device="cuda:0")
    assert _triples_equal(ix.search_f32_device(_dev(qrows), 25), ix.search_device(qi, qs, 25))
    assert torch.equal(ix.score_docs_f32_device(_dev(qrows), cand), ix.score_docs_device(qi, qs, cand))
    ux = sparse_rx.DenseUint8Index.from_embeddings(rows)
    uq = [sparse_rx.quantize_query_asymmetric(q) for q in qrows]
    qf = ux._queries_to_device(np.stack([a for a, _ in uq]), np.stack([b for _, b in uq]))
    assert _triples_equal(ux.search_raw_device(_dev(qrows), 25), ux.search_device(qf, 25))
    assert torch.equal(ux.score_docs_raw_device(_dev(qrows), cand), ux.score_docs_device(qf, cand))
    # a flagged query (all zero / non-finite) is an empty row, not an error
    z = qrows[:3].copy()
    z[0], z[1, 5] = 0, np.nan
    d, s, c = ix.search_f32_device(_dev(z), 5)
    assert c.tolist()[:2] == [0, 0] and c[2].item() == 5 and (d[:2] == -1).all().item()
    with pytest.raises(ValueError, match="float32"):
        ix.search_f32_device(_dev(qrows).double(), 5)


def test_quantized_embedding_index_device_equals_host_and_the_fixture(fixtures):
    z, _, j = fixtures
    host, dev = sparse_rx.QuantizedEmbeddingIndex(), sparse_rx.QuantizedEmbeddingIndex(quantize="device")
    host.build(j["doc_ids"], z["emb"])
    dev.build(j["doc_ids"], z["emb"])
    qembs = {qid: z["qemb"][i] for i, qid in enumerate(j["qids"])}
    for k_s, res in j["results"].items():
        got = dev.search(qembs, top_k=int(k_s))
        exp = host.search(qembs, top_k=int(k_s))
        assert got == exp and [list(g) for g in got.values()] == [list(e) for e in exp.values()]
        for qid in j["qids"]:
            assert list(got[qid].values()) == list(res[qid].values())  # tests/golden/dense_int8.json, score by score
    assert dev.search({}, top_k=5) == {}
    with pytest.raises(ValueError, match="float32"):
        dev.search({q: e.astype(np.float64) for q, e in qembs.items()}, top_k=5)
    with pytest.raises(ValueError, match="float32"):
        sparse_rx.QuantizedEmbeddingIndex(quantize="device").build(j["doc_ids"], z["emb"].astype(np.float64))


def _same_dicts(a, b):
    return a == b and list(a) == list(b) and all(list(a[q]) == list(b[q]) for q in a)


@pytest.mark.parametrize("scheme", ("symmetric", "asymmetric"))
def test_quantized_embedding_retriever_device_equals_host(scheme):
    corpus = {f"doc{i}": {"text": f"t{i}"} for i in range(400)}
    mk = lambda quantize: sparse_rx.RetrieverRegistry.create({"type": "dpr", "params": {"embedding_dim": 100, "quantization_method": scheme,
                                                                                         "quantize": quantize}})
    host, dev = mk("host"), mk("device")
    host.build_index_from_corpus(corpus)
    dev.build_index_from_corpus(corpus)
    assert dev._corpus_codes is None  # nothing was copied back yet
    queries = {"a": "alpha beta", "b": "gamma", "blank": "", "c": "delta epsilon zeta"}
    assert _same_dicts(dev.search(queries, top_k=30), host.search(queries, top_k=30))  # same process: same hash(text) seeds
    qemb = {f"q{i}": host.query_embedding_from_seed(50 + i) for i in range(9)}
    cands = {q: [f"doc{(7 * i + 3 * t) % 400}" for t in range(1 + i)] for i, q in enumerate(qemb)}
    cands["q4"] = []
    assert _same_dicts(dev.score(qemb, cands), host.score(qemb, cands))
    assert same_bits(dev.corpus_embeddings_int8, host.corpus_embeddings_int8) and same_bits(dev.corpus_scales, host.corpus_scales)
    assert dev.corpus_embeddings_int8 is dev.corpus_embeddings_int8  # copied back once


def test_hybrid_retriever_device_equals_host():
    torch = _torch()
    from sparse_rx import synth
    corpus, queries = synth.fiqa_shaped_text(n_docs=3000, vocab=4000, mean_doc_len=40, n_queries=10, seed=9)
    queries = dict(queries)
    queries["blank"] = ""
    queries["oov"] = "zzzunknown qqqmissing"
    emb = np.random.default_rng(3).standard_normal((len(corpus), 48)).astype(np.float32)
    mk = lambda quantize, **kw: sparse_rx.RetrieverRegistry.create({"type": "hybrid", "model": {"sparse": "bm25_custom", "dense": "dpr"},
                                                                    "params": {"embedding_dim": 48, "quantize": quantize, **kw}})
    host, dev = mk("host"), mk("device")
    host.build_index_from_corpus(corpus, embeddings=emb)
    dev.build_index_from_corpus(corpus, embeddings=emb)
    assert torch.equal(dev.dense._index.corpus, host.dense._index.corpus) and torch.equal(dev.dense._index.scales, host.dense._index.scales)
    qemb = {qid: host.dense.query_embedding_from_seed(100 + i) for i, qid in enumerate(queries)}
    block = np.stack([qemb[q] for q in queries])  # row i = the i-th key of ``queries``, the blank one included
    for r in (host, dev):
        r.candidates = 100
    for fusion, rescore in (("weighted", False), ("rrf", False), ("weighted", True)):
        for r in (host, dev):
            r.fusion, r.rescore = fusion, rescore
        exp = host.search(queries, top_k=20, query_embeddings=qemb)
        assert exp["blank"] == {} and len(exp["oov"]) == 20
        assert _same_dicts(dev.search(queries, top_k=20, query_embeddings=qemb), exp)
        assert _same_dicts(dev.search(queries, top_k=20, query_embeddings=_dev(block)), exp)  # a device tensor, never on the host
        assert _same_dicts(dev.search(queries, top_k=20, query_embeddings=block), exp)
        assert _same_dicts(host.search(queries, top_k=20, query_embeddings=_dev(block)), exp)
    assert same_bits(dev.dense.corpus_embeddings_int8, host.dense.corpus_embeddings_int8)
    with pytest.raises(ValueError, match="shape"):
        dev.search(queries, top_k=5, query_embeddings=_dev(block[:-1]))
    with pytest.raises(ValueError, match="float32"):
        dev.search(queries, top_k=5, query_embeddings=_dev(block).double())
    host.close()
    dev.close()
