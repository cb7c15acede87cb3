"""The half-precision dense index on the GPU (include/sparse_rx_half.h), both types.  The conversion is compared byte for
byte with the NumPy restatement (tests/half_ref.py).  The scores of one MFMA chain cannot be restated bit for bit (the order
and rounding inside the instruction are the hardware's), so they are pinned from three sides: integer operands, where every
order gives the same exact result, must match NumPy to the bit; on random data every score lies within the derived bound
tol(q, d) = dim_pad * 2^-22 * sum |q_i d_i| of the fp64 dot product of the rounded operands; and the bits of a (query, doc)
pair are the same from the search, from the scorer of given docs, alone or in a batch, wherever the doc's row sits, and on a
second run.  Rankings are tests/parity.py's dense_topk_rows of those scores."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import half_ref  # noqa: E402
import hybrid_ref  # noqa: E402
import parity  # noqa: E402
from test_gpu_parity import _assert_exact  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = ["f16", "bf16"]
BASE = 7_000_000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()


def _pad64(dim):
    return (dim + 63) // 64 * 64


def _corpus_codes(ix):
    """The resident buffer as u16, as the device holds it."""
    import torch
    torch.cuda.synchronize()
    return ix.corpus.cpu().numpy().view(np.uint16)


def _special_rows(rng, n, dim, dtype):
    """Random normal rows with the values rounding has to get right sprinkled in: ties of the type, half subnormals, -0.0."""
    e = rng.standard_normal((n, dim)).astype(np.float32)
    if dtype == "f16":
        special = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 6e-8, -6e-8, 1e-6,
                            65504.0, 65519.0, -0.0, 0.0, 2.0 ** -14 - 2.0 ** -25], np.float32)
    else:
        special = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00008000, 0x00018000, 0x3F807FFF, 0x3F808001, 0x00000001, 0x80000000,
                            0x00000000, 0x7F7F0000, 0x00400000, 0x80400001], np.uint32).view(np.float32)
    flat = e.reshape(-1)
    pos = rng.choice(flat.size, size=min(flat.size, 4 * len(special)), replace=False)
    flat[pos] = special[np.arange(len(pos)) % len(special)]
    return e


# ---- 1. conversion: bytes against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_convert_every_row_length(dtype):
    import torch
    import sparse_rx
    rng = np.random.default_rng(41)
    for dim in (1, 3, 63, 64, 65, 200, 768, 1000, 1024):
        for n in (1, 31, 32, 33, 1000):
            e = _special_rows(rng, n, dim, dtype)
            codes, flag = half_ref.convert(e, dtype, _pad64(dim))
            assert flag == 0
            exp = half_ref.pack(codes)
            ix = sparse_rx.DenseHalfIndex(torch.as_tensor(e, device="cuda:0"), dtype=dtype)  # ld == dim, one launch
            assert (ix.n_docs, ix.dim, ix.dim_pad, ix.device_bytes()) == (n, dim, _pad64(dim), exp.nbytes)
            assert np.array_equal(_corpus_codes(ix), exp), f"{dtype} dim={dim} n={n}"
            if n == 33:
                assert np.array_equal(ix.corpus_to_host(), codes[:, :dim])


def _junk(n, value):
    import torch
    return torch.as_tensor(np.full(n, value, np.uint16).view(np.int16), device="cuda:0")


def _convert_raw(x, dtype, dim_pad, row0, n_total, out, flag):
    """srx_dense_convert_half on the current stream; x: a device view with unit column stride."""
    import torch
    from sparse_rx import _capi
    from sparse_rx.index import _stream_ptr
    n, dim = x.shape
    rc = _capi.lib().srx_dense_convert_half(0, half_ref.TYPES[dtype], x.data_ptr(), x.stride(0) if n > 1 else dim, n, dim, dim_pad, row0, n_total,
                                            out.data_ptr(), None if flag is None else flag.data_ptr(), _stream_ptr(torch, out.device))
    _capi.check(rc, "srx_dense_convert_half")


@pytest.mark.parametrize("dtype", DTYPES)
def test_convert_slice_chunks_junk_and_stream(dtype):
    import torch
    rng = np.random.default_rng(42)
    n, dim = 1000, 200
    dim_pad = _pad64(dim)
    e = _special_rows(rng, n, dim, dtype)
    exp = half_ref.pack(half_ref.convert(e, dtype, dim_pad)[0])
    junk = 0xABCD
    # a column slice of a wider tensor: ld = dim + 3, the base 4 bytes off a 16-byte boundary; the output pre-filled with junk
    wide = torch.zeros((n, dim + 3), dtype=torch.float32, device="cuda:0")
    wide[:, 1: dim + 1] = torch.as_tensor(e, device="cuda:0")
    x = wide[:, 1: dim + 1]
    assert x.stride(0) == dim + 3 and x.data_ptr() % 16 == 4
    out = _junk(exp.size, junk)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    _convert_raw(x, dtype, dim_pad, 0, n, out, flag)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), exp) and int(flag.item()) == 0
    # chunks: the first and the last, then the middle one; each leaves the other tiles alone.  flag = NULL is legal
    out = _junk(exp.size, junk)
    full = torch.as_tensor(e, device="cuda:0")
    per_tile = 32 * dim_pad
    _convert_raw(full[:320], dtype, dim_pad, 0, n, out, None)
    _convert_raw(full[640:], dtype, dim_pad, 640, n, out, None)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert (got[10 * per_tile: 20 * per_tile] == junk).all(), "the first and last chunk wrote into the middle tiles"
    assert np.array_equal(got[: 10 * per_tile], exp[: 10 * per_tile]) and np.array_equal(got[20 * per_tile:], exp[20 * per_tile:])
    _convert_raw(full[320:640], dtype, dim_pad, 320, n, out, None)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), exp)
    # a middle chunk that ends inside a tile writes zeros for the tile's other rows (the header: only the last chunk may)
    out = _junk(exp.size, junk)
    _convert_raw(full[320:330], dtype, dim_pad, 320, n, out, None)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    tile = half_ref.unpack(got[10 * per_tile: 11 * per_tile], 32, dim_pad)
    assert np.array_equal(tile[:10], half_ref.convert(e[320:330], dtype, dim_pad)[0]) and not tile[10:].any()
    assert (got[: 10 * per_tile] == junk).all() and (got[11 * per_tile:] == junk).all()
    # a side stream, through the class, from a host array in chunks of 64 rows
    import sparse_rx
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ix = sparse_rx.DenseHalfIndex.from_embeddings(e, dtype=dtype, chunk_rows=64, doc_base=5)
    s.synchronize()
    assert np.array_equal(_corpus_codes(ix), exp) and ix.doc_base == 5
    with pytest.raises(ValueError, match="multiple of 32"):
        sparse_rx.DenseHalfIndex(e, dtype=dtype, chunk_rows=48)


@pytest.mark.parametrize("dtype", DTYPES)
def test_convert_non_finite_rows(dtype):
    import torch
    import sparse_rx
    rng = np.random.default_rng(43)
    n, dim = 70, 65
    e = rng.standard_normal((n, dim)).astype(np.float32)
    e[3, 64] = np.nan
    e[40, 0] = 70000.0  # finite as bf16, not as f16
    e[69, 7] = -np.inf
    e[5, 5] = 3.4e38    # rounds to inf in both types
    codes, flag = half_ref.convert(e, dtype, 128)
    assert flag == 1 and not codes[3].any() and not codes[69].any() and not codes[5].any() and bool(codes[40].any()) == (dtype == "bf16")
    out = torch.full((half_ref.half_bytes(n, 128) // 2,), 0x1234, dtype=torch.int16, device="cuda:0")
    fl = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    _convert_raw(torch.as_tensor(e, device="cuda:0"), dtype, 128, 0, n, out, fl)
    torch.cuda.synchronize()
    assert int(fl.item()) == 1
    assert np.array_equal(out.cpu().numpy().view(np.uint16), half_ref.pack(codes))
    with pytest.raises(ValueError, match="not finite"):
        sparse_rx.DenseHalfIndex(e, dtype=dtype)
    ok = e.copy()
    ok[[3, 69, 5]] = 1.0
    ok[40, 0] = 60000.0
    sparse_rx.DenseHalfIndex(ok, dtype=dtype)  # a clean matrix sets no flag


# ---- 2. exact arithmetic: integers in [-3, 3] ----------------------------------------------------------------------------------
def _int_case(n, nq, dim, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    q = rng.integers(-3, 4, (nq, dim)).astype(np.float32)
    q[0] = 0.0  # scores nothing > 0: count 0, a padded row
    if nq > 2:
        q[2] = -np.abs(q[2])
    return d, q, (q.astype(np.float64) @ d.astype(np.float64).T).astype(np.float32)  # |score| <= 9 * 1024: exact in any order


def _expected(S, k, base):
    d, s, c = parity.dense_topk_rows(S, k)
    return np.where(d >= 0, d + base, d).astype(np.int32), s, c


INT_CASES = [(1, 1, 1, 1, 0), (31, 31, 64, 10, 0), (32, 32, 65, 1024, BASE), (33, 33, 1024, 10, 0), (127, 129, 64, 1024, 0), (128, 1, 65, 1, BASE),
             (129, 32, 1024, 10, 0), (4099, 33, 64, 1024, BASE), (4099, 129, 1024, 10, 0), (4099, 31, 1, 10, 0), (4099, 1025, 64, 10, 0),
             (32801, 5, 64, 100, BASE)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nq,dim,k,base", INT_CASES)
def test_exact_on_small_integers(dtype, n, nq, dim, k, base):
    import sparse_rx
    d, q, S = _int_case(n, nq, dim, seed=n * 7 + nq)
    if n == 32801:
        assert parity.dense_splits(n, nq, k) == 2, "the rank kernel should run 2 splits"
    ix = sparse_rx.DenseHalfIndex(d, dtype=dtype, doc_base=base)
    exp = _expected(S, k, base)
    assert exp[2][0] == 0 and (n < 4099 or (exp[2][1:] > 0).any())
    _assert_exact(ix.search(q, k), exp, f"{dtype} n={n} nq={nq} dim={dim} k={k}")
    # the scorer of given docs on the same pairs: every doc, in reverse order
    cand = np.tile(np.arange(n - 1, -1, -1, dtype=np.int32) + base, (nq, 1))[:, :4099]
    got = ix.score_docs(q, cand)
    assert np.array_equal(got.view(np.uint32), (S[:, ::-1][:, :4099] + np.float32(0.0)).view(np.uint32))


# ---- 3. random normal data -------------------------------------------------------------------------------------------------------
SHAPES = [(32801, 128), (4099, 200), (32801, 768)]
NQ = 33


class _Random:
    """Per (shape, type): the corpus, 33 queries, the index, S = score_docs of every (query, doc) pair -- computed once, read-only."""

    def __init__(self):
        self.cache = {}

    def get(self, shape, dtype):
        import sparse_rx
        key = (shape, dtype)
        if key not in self.cache:
            n, dim = shape
            rng = np.random.default_rng(1000 + n + dim)
            emb = rng.standard_normal((n, dim)).astype(np.float32)
            q = rng.standard_normal((NQ, dim)).astype(np.float32)
            ix = sparse_rx.DenseHalfIndex(emb, dtype=dtype, doc_base=BASE)
            S = ix.score_docs(q, np.tile(np.arange(n, dtype=np.int32) + BASE, (NQ, 1)))
            for a in (emb, S):  # q goes to torch.as_tensor as it is, which wants a writable array
                a.setflags(write=False)
            self.cache[key] = (emb, q, ix, S)
        return self.cache[key]


@pytest.fixture(scope="module")
def rnd():
    return _Random()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_random_scores_within_the_bound(rnd, shape, dtype):
    emb, q, ix, S = rnd.get(shape, dtype)
    dim_pad = _pad64(shape[1])
    dc, _ = half_ref.convert(emb, dtype, dim_pad)
    qc, _ = half_ref.convert(q, dtype, dim_pad)
    exact, tol = half_ref.exact_scores(qc, dc, dtype), half_ref.tol(qc, dc, dtype)
    err = np.abs(S.astype(np.float64) - exact)
    rel = float((err / half_ref.abs_scores(qc, dc, dtype)).max())
    print(f"half {dtype} {shape}: max |S - exact| / sum|q d| = {rel:.3e} (bound {dim_pad * 2.0 ** -22:.3e})")
    assert (err <= tol).all(), f"{dtype} {shape}: {int((err > tol).sum())} scores outside the bound, worst ratio {rel:.3e}"
    assert (S < 0).any() and (S > 0).any()
    # the index's own view of its rows
    assert np.array_equal(ix.corpus_to_host(), dc[:, : shape[1]])
    assert abs(ix.max_row_norm() - float(np.sqrt((half_ref.to_f32(dc, dtype).astype(np.float64) ** 2).sum(axis=1).max()))) < 1e-9


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_search_is_the_ranking_of_the_scorers_bits(rnd, shape, dtype):
    """Two different kernels (the GEMM and the gathering scorer) agree on every bit; a query's bits do not depend on the batch."""
    emb, q, ix, S = rnd.get(shape, dtype)
    for k in (10, 100, 1024):
        rows33 = ix.search(q, k)
        _assert_exact(rows33, _expected(S, k, BASE), f"{dtype} {shape} k={k} nq=33")
        _assert_exact(ix.search(q[:5], k), _expected(S[:5], k, BASE), f"{dtype} {shape} k={k} nq=5")
    alone = ix.search(q[7], 100)
    batch = ix.search(q, 100)
    _assert_exact(alone, tuple(a[7:8] for a in batch), f"{dtype} {shape} query 7 alone vs in the batch")
    _assert_exact(ix.search(q, 100), batch, "second run")
    S2 = ix.score_docs(q, np.tile(np.arange(shape[0], dtype=np.int32) + BASE, (NQ, 1)))
    assert np.array_equal(S2.view(np.uint32), S.view(np.uint32)), "second run of the scorer"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_score_bits_do_not_depend_on_the_row(rnd, shape, dtype):
    """Doc row 100 copied to rows 0, 31, 32 and n_docs - 1 of a second index scores to the same bits there: from the scorer
    for the 33 random queries, and from the GEMM for queries built on the row itself, which put all five copies at the top
    of the ranking (score about |row|^2 = dim, the other docs about sqrt(dim)), so every one of them IS compared."""
    import sparse_rx
    emb, q, ix, S = rnd.get(shape, dtype)
    n = shape[0]
    src, places = 100, [0, 31, 32, n - 1]
    moved = emb.copy()
    moved[places] = emb[src]
    ix2 = sparse_rx.DenseHalfIndex(moved, dtype=dtype)
    got = ix2.score_docs(q, np.tile(np.array(places, np.int32), (NQ, 1)))
    assert np.array_equal(got.view(np.uint32), np.repeat(S[:, src: src + 1], len(places), axis=1).view(np.uint32))
    own = np.stack([emb[src], 0.5 * emb[src] + 0.1 * q[0], emb[src] + 0.3 * q[1], 0.75 * emb[src] - 0.2 * q[2], 1.5 * emb[src] - 0.1 * q[3]]).astype(np.float32)
    want = ix.score_docs(own, np.full((len(own), 1), src + BASE, np.int32))  # the pair's bits in the first index, doc at row 100
    d, s, c = ix2.search(own, 10)
    copies = sorted(places + [src])
    for i in range(len(own)):
        assert c[i] == 10 and d[i, :5].tolist() == copies, f"query {i}: the five copies should lead, doc ascending: {d[i]}"
        assert (s[i, :5].view(np.uint32) == want[i, 0].view(np.uint32)).all() and s[i, 5] < s[i, 4]
    # ... and in a batch with the random queries, from a different query tile position
    both = np.concatenate([q, own])
    d, s, c = ix2.search(both, 10)
    assert (d[NQ:, :5] == np.array(copies)).all() and (s[NQ:, :5].view(np.uint32) == want.view(np.uint32)).all()


# ---- 4. the scorer of given docs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_score_docs_contract(rnd, dtype):
    import torch
    emb, q, ix, S = rnd.get(SHAPES[1], dtype)
    n = SHAPES[1][0]
    rng = np.random.default_rng(44)
    m = 70
    local = rng.integers(0, n, (NQ, m))
    local[:, 5] = local[:, 4]  # duplicates
    local[:, 6] = local[:, 4]
    cand = (local + BASE).astype(np.int32)
    dead = {10: -1, 11: BASE - 1, 12: BASE + n, 13: 0, 14: 2 ** 31 - 1, 69: -1}
    for c, v in dead.items():
        cand[:, c] = v
    exp = np.take_along_axis(S, local, axis=1).copy()
    exp[:, list(dead)] = 0.0
    got = ix.score_docs(q, cand)  # cand_count = NULL
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert (got < 0).any(), "negative scores are returned"
    counts = (np.arange(NQ) * 3 % (m + 1)).astype(np.int32)
    counts[1] = 0
    exp_c = np.where(np.arange(m)[None, :] < counts[:, None], exp, np.float32(0.0))
    got_c = ix.score_docs(q, cand, counts)
    assert np.array_equal(got_c.view(np.uint32), exp_c.view(np.uint32))
    # a search result block passed back as it is (device tensors, -1 padded, with its counts): its own scores, +0 in the padding
    import sparse_rx
    qd = torch.as_tensor(q, device=ix.device)
    few = sparse_rx.DocFilter.from_masks(np.random.default_rng(47).random(n) < 0.01, doc_base=BASE)  # ~ 40 allowed docs: short, padded rows
    for flt in (None, few):
        d, s, c = ix.search_device(qd, 1024, filter=flt)
        out = torch.full((NQ, 1024), 7.0, dtype=torch.float32, device=ix.device)
        back = ix.score_docs_device(qd, d, c, out=out)
        torch.cuda.synchronize()
        assert back is out and (flt is None or (c.cpu().numpy() < 1024).all())
        assert np.array_equal(back.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint32))
        assert np.array_equal(ix.score_docs_device(qd, d).cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint32))


# ---- 5. filters ----------------------------------------------------------------------------------------------------------------
def _masks(n_docs, densities, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.ones(n_docs, bool) if d >= 1 else np.zeros(n_docs, bool) if d <= 0 else rng.random(n_docs) < d for d in densities])


def _filtered_expected(S, masks, q_filter, k):
    s = S.copy()
    for i, r in enumerate(q_filter):
        if r >= 0:
            s[i, ~masks[r]] = 0.0  # a disallowed column is never a result: only scores > 0 are
    return _expected(s, k, BASE)


@pytest.mark.parametrize("dtype", DTYPES)
def test_filtered_search(rnd, dtype):
    import sparse_rx
    emb, q, ix, S = rnd.get(SHAPES[0], dtype)
    n = SHAPES[0][0]
    assert parity.dense_splits(n, NQ, 100) == 2
    masks = _masks(n, [1.0, 0.0, 0.5, 0.01], seed=45)
    flt = sparse_rx.DocFilter.from_masks(masks, doc_base=BASE)
    q_filter = np.array([(-1, 0, 1, 2, 3)[i % 5] for i in range(NQ)], np.int32)
    for k in (10, 100):
        exp = _filtered_expected(S, masks, q_filter, k)
        _assert_exact(ix.search(q, k, filter=flt, q_filter=q_filter), exp, f"{dtype} filtered k={k}")
        assert (exp[2][q_filter == 1] == 0).all() and (exp[2][q_filter == 3] > 0).all()
    # q_filter = None: row 0 for every query, the unfiltered rows
    _assert_exact(ix.search(q, 100, filter=flt), _expected(S, 100, BASE), f"{dtype} row 0 for all")
    half_only = sparse_rx.DocFilter.from_masks(masks[2], doc_base=BASE)
    _assert_exact(ix.search(q, 100, filter=half_only), _filtered_expected(S, masks[2:3], np.zeros(NQ, np.int32), 100), f"{dtype} one row, q_filter None")
    # exactly six docs, then their complement
    allowed = np.array([0, 31, 32, 1023, 1024, n - 1])
    only = np.zeros(n, bool)
    only[allowed] = True
    two = np.stack([only, ~only])
    flt2 = sparse_rx.DocFilter.from_masks(two, doc_base=BASE)
    qf2 = (np.arange(NQ) % 2).astype(np.int32)
    pos = np.abs(q) * np.sign(emb[allowed].mean(axis=0))  # a second batch, leaning towards the six docs: more of them score > 0
    for queries, Sq in ((q, S), (pos.astype(np.float32), None)):
        if Sq is None:
            Sq = ix.score_docs(queries, np.tile(np.arange(n, dtype=np.int32) + BASE, (NQ, 1)))
        exp = _filtered_expected(Sq, two, qf2, 100)
        _assert_exact(ix.search(queries, 100, filter=flt2, q_filter=qf2), exp, f"{dtype} six docs / complement")
        assert set(exp[0][qf2 == 0].ravel().tolist()) - {-1} <= set((allowed + BASE).tolist())
    with pytest.raises(ValueError):
        ix.search(q, 10, filter=sparse_rx.DocFilter.from_masks(masks[:, :-1], doc_base=BASE))
    with pytest.raises(ValueError):
        ix.search(q, 10, q_filter=q_filter)


# ---- 6. score_offset -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_score_offset_ranks_every_doc(rnd, dtype):
    emb, q, ix, S = rnd.get(SHAPES[1], dtype)
    n = SHAPES[1][0]
    off = np.float32(np.ceil(np.abs(S).max()) + 1.0)  # above max |S|: every shifted value is > 0
    shifted = S + off  # fp32 + fp32: fl32(score + offset)
    assert shifted.dtype == np.float32 and (shifted > 0).all()
    for k in (100, 1024):
        exp = _expected(shifted, k, BASE)
        assert (exp[2] == k).all()
        _assert_exact(ix.search(q, k, score_offset=float(off)), exp, f"{dtype} offset k={k}")
    small = ix.search(emb[:5] * 0.01, n if n <= 1024 else 1024, score_offset=float(off))
    assert (small[2] == 1024).all()


# ---- 7. the service --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "text_small.json"), encoding="utf-8") as f:
        return json.load(f)


def test_service_with_half_storage(golden):
    import rescore_ref
    import sparse_rx
    from test_hybrid_gpu import _assert_dicts, _rows_from_dicts
    j = golden
    queries = dict(j["queries"])
    live = [q for q in queries if queries[q].strip()]
    dim, n_docs = 96, len(j["corpus"])
    rng = np.random.default_rng(46)
    emb = rng.standard_normal((n_docs, dim)).astype(np.float32)
    vecs = {q: rng.standard_normal(dim).astype(np.float32) for q in queries}
    svc = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    svc.build_bm25_index(j["corpus"])
    svc.set_embeddings(emb, storage="f16")
    assert isinstance(svc._dense, sparse_rx.DenseHalfIndex) and svc._dense.dtype == "f16" and svc.get_stats()["embedding_storage"] == "f16"
    row_of = {d: i for i, d in enumerate(svc.doc_ids)}
    # the dense scores of every pair: within the bound of the rounded operands' exact dot products
    Q = np.stack([vecs[q] for q in live])
    S = svc._dense.score_docs(Q, np.tile(np.arange(n_docs, dtype=np.int32), (len(live), 1)))
    dc, _ = half_ref.convert(emb, "f16", 128)
    qc, _ = half_ref.convert(Q, "f16", 128)
    assert (np.abs(S - half_ref.exact_scores(qc, dc, "f16")) <= half_ref.tol(qc, dc, "f16")).all()
    # search_by_vector: the ranking of those scores (first pass: k rows > 0)
    got = svc.search_by_vector(vecs[live[0]], k=5)
    d, s, c = parity.dense_topk_rows(S[:1], 5)
    assert c[0] == 5 and [r["doc_id"] for r in got] == [svc.doc_ids[i] for i in d[0]]
    assert np.array_equal(np.array([r["score"] for r in got], np.float32).view(np.uint32), s[0].view(np.uint32))
    # ... with excluded docs; and the second pass (min_score <= 0, fewer than k positive scores) re-scores with the f32 rows
    shown = [r["doc_id"] for r in got[:2]]
    got_x = svc.search_by_vector(vecs[live[0]], k=5, excluded_docs=shown)
    Sx = S[:1].copy()
    Sx[0, [row_of[x] for x in shown]] = 0.0
    d, s, c = parity.dense_topk_rows(Sx, 5)
    assert [r["doc_id"] for r in got_x] == [svc.doc_ids[i] for i in d[0]] and not set(shown) & {r["doc_id"] for r in got_x}
    kk = min(n_docs, 1000)
    allk = svc.search_by_vector(vecs[live[0]], k=kk, min_score=-1e9)
    f32 = np.dot(emb.astype(np.float64), vecs[live[0]].astype(np.float64))
    sc = np.array([r["score"] for r in allk])
    assert len(allk) == kk and (np.diff(sc) <= 0).all() and sc.min() < 0
    assert np.abs(sc - f32[[row_of[r["doc_id"]] for r in allk]]).max() < 1e-4  # fp32 dot products of the f32 rows, not half scores
    # score_by_vector: the scorer's bits
    cands = {q: [svc.doc_ids[(3 * i + t) % n_docs] for t in range(4)] for i, q in enumerate(live)}
    sv = svc.score_by_vector({q: vecs[q] for q in live}, cands)
    for i, q in enumerate(live):
        assert list(sv[q]) == cands[q]
        assert np.array_equal(np.array(list(sv[q].values()), np.float32).view(np.uint32), S[i, [row_of[x] for x in cands[q]]].view(np.uint32))
    # search_hybrid, plain and rescored, with excluded docs: the fusion (hybrid_ref / rescore_ref) of the two filtered lists
    excluded = [x for i, x in enumerate(svc.doc_ids) if i % 2 == 0]
    mask = np.ones(n_docs, bool)
    mask[[row_of[x] for x in excluded]] = False
    flt = sparse_rx.DocFilter.from_masks(mask)
    k, cdepth = 10, 20
    Sm = S.copy()
    Sm[:, ~mask] = 0.0
    for rescore in (False, True):
        got = svc.search_hybrid(queries, vecs, top_k=k, candidates=cdepth, excluded_docs=excluded, rescore=rescore)
        assert all(got[q] == {} for q in queries if q not in live) and any(got[q] for q in live)
        assert all(not set(got[q]) & set(excluded) for q in live)
        sparse = _rows_from_dicts(svc.search_bm25(queries, top_k=cdepth, excluded_docs=excluded), live, row_of, cdepth)
        dense = svc._dense.search(Q, cdepth, filter=flt)
        _assert_exact(dense, parity.dense_topk_rows(Sm, cdepth), "the dense side's filtered lists")
        if not rescore:
            _assert_dicts(got, live, hybrid_ref.fuse(sparse, dense, k, "weighted", (0.3, 0.7)), svc.doc_ids)
        else:
            qa = sparse_rx.encode_queries([queries[q] for q in live], svc.host.vocabulary)
            a_other = np.where(sparse[0] >= 0, np.take_along_axis(S, np.maximum(sparse[0], 0), axis=1), np.float32(0.0))
            a_other = np.where(np.arange(cdepth)[None, :] < sparse[2][:, None], a_other, np.float32(0.0)).astype(np.float32)
            assert np.array_equal(svc._dense.score_docs(Q, sparse[0], sparse[2]).view(np.uint32), a_other.view(np.uint32))
            b_other = svc.dev.score_docs(*qa, dense[0], dense[2])
            _assert_dicts(got, live, rescore_ref.fuse_scored(sparse, a_other, dense, b_other, k, (0.3, 0.7)), svc.doc_ids)
    plain = svc.search_hybrid(queries, vecs, top_k=k, candidates=cdepth)
    sparse = _rows_from_dicts(svc.search_bm25(queries, top_k=cdepth), live, row_of, cdepth)
    _assert_dicts(plain, live, hybrid_ref.fuse(sparse, parity.dense_topk_rows(S, cdepth), k, "weighted", (0.3, 0.7)), svc.doc_ids)
    svc.close()

    # storage="f32" (and the default): the calls return what they return without the keyword
    a = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    b = sparse_rx.RetrievalService(device="cuda:0", tile_log2=6)
    for s_, kw in ((a, {}), (b, {"storage": "f32"})):
        s_.build_bm25_index(j["corpus"])
        s_.set_embeddings(emb, **kw)
        assert isinstance(s_._dense, sparse_rx.DenseF32Index) and s_.get_stats()["embedding_storage"] == "f32"
    sims = parity.dense_rows_scores(np.pad(emb, ((0, 0), (0, 128 - dim))), np.pad(vecs[live[0]], (0, 128 - dim))[None, :])
    d, s, c = parity.dense_topk_rows(sims, 5)
    for s_ in (a, b):
        got = s_.search_by_vector(vecs[live[0]], k=5)
        assert [r["doc_id"] for r in got] == [s_.doc_ids[i] for i in d[0, : c[0]]]
        assert np.array_equal(np.array([r["score"] for r in got], np.float32).view(np.uint32), s[0, : c[0]].view(np.uint32))
    for rescore in (False, True):
        assert a.search_hybrid(queries, vecs, top_k=k, candidates=cdepth, excluded_docs=excluded, rescore=rescore) == \
            b.search_hybrid(queries, vecs, top_k=k, candidates=cdepth, excluded_docs=excluded, rescore=rescore)
    assert a.score_by_vector({q: vecs[q] for q in live}, cands) == b.score_by_vector({q: vecs[q] for q in live}, cands)
    a.close()
    b.close()


def test_search_by_vector_shift_covers_the_rounded_query():
    """bf16 rounding can raise every component of a query by almost 2^-8 of itself (here 1 + 2^-8 + 2^-20 -> 1 + 2^-7), so the
    rounded query's norm exceeds |q|_2 by 0.39 %.  The doc of largest norm, anti-parallel to it, then scores below
    -|q|_2 * max_row_norm: the second pass of search_by_vector must still rank it (every doc is rankable: n_docs rows)."""
    import sparse_rx
    n, dim = 64, 64
    rng = np.random.default_rng(48)
    q = np.full(dim, 1.0 + 2.0 ** -8 + 2.0 ** -20, np.float32)
    qr = half_ref.to_f32(half_ref.round_bf16(q), "bf16")
    assert (qr == np.float32(1.0 + 2.0 ** -7)).all()
    emb = (0.01 * rng.standard_normal((n, dim))).astype(np.float32)
    emb[5] = -qr  # exact in bf16: the row of largest norm, score -64 (1 + 2^-7)^2
    svc = sparse_rx.RetrievalService(device="cuda:0")
    svc.set_embeddings(emb, storage="bf16")
    assert float(np.linalg.norm(qr.astype(np.float64))) * svc._dense.max_row_norm() > 1.001 * float(np.linalg.norm(q.astype(np.float64))) * svc._dense.max_row_norm()
    got = svc.search_by_vector(q, k=n, min_score=-1e9)
    assert len(got) == n and got[-1]["doc_id"] == "5" and got[-1]["score"] < -64.0
    svc.close()
