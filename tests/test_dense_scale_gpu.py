"""The dense kernels past 2^31 / 2^32 bytes and elements, and the large-corpus branches of the INT8 pass plan, on the device.

Every case is a row of tests/dense_scale.py.  The corpus is a zero-filled extent of ONE device arena (allocated once for the
module at the size of the largest case, never a host array); only the planted rows hold values, written in the stored form
through the layout restatements the suite already has (rescore_ref.pack_i8, half_ref.pack, binary_ref.tile).  Zero rows score
exactly 0 and are no result, so the expected rows of a search are the ranking of the planted rows by the existing bit-exact
restatements -- O(planted x dim) on the host.  Calls go through the C ABI with the test's own buffers; outputs and
workspaces are pre-filled with 0x7F7F7F7F and the 64 words behind every workspace must still hold it.  Every comparison is
exact.  In every case one batch runs with doc_base + n_docs == 2^31 - 2, the largest the checks allow.

Wall times and peak memory of every test go to the file SRX_DENSE_SCALE_LOG names, if it is set (profiles/dense_scale_tests.log
is such a run)."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import binary_ref  # noqa: E402
import dense_scale as T  # noqa: E402
import filter_ref  # noqa: E402
import half_ref  # noqa: E402
import late_ref  # noqa: E402
import quant_ref  # noqa: E402
import rescore_ref  # noqa: E402
from oracle import np_oracle  # noqa: E402  (checker only)
from parity import dense_plan, dense_plan_label, dense_rows_scores, dense_topk_rows, dense_ws  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
GARBAGE = T.GARBAGE
CASES = {c.name: c for c in T.CASES + T.PLAN_CASES}


# ---- the arena, the call wrapper, the log ---------------------------------------------------------------------------------------
class Arena:
    """One device allocation, handed out in 256-byte aligned pieces; reset() before every case."""

    def __init__(self, nbytes):
        import torch
        try:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        except Exception as e:  # a failed allocation is a failure, not a skip
            free, total = torch.cuda.mem_get_info()
            pytest.fail(f"the arena of {nbytes} bytes could not be allocated: torch.cuda.mem_get_info() = ({free}, {total}): {e}")
        self.off = 0

    def reset(self):
        self.off = 0

    def take(self, nbytes, dtype=None, fill=None):
        """nbytes of the arena as a tensor of dtype; fill: None (as it is), 0, or GARBAGE (every 32-bit word)"""
        import torch
        off = T.r256(self.off)
        assert nbytes % 4 == 0 and off + nbytes <= self.buf.numel(), f"the arena is too small: {off} + {nbytes} > {self.buf.numel()}"
        self.off = off + nbytes
        t = self.buf[off: off + nbytes]
        if fill == 0:
            t.zero_()
        elif fill is not None:
            t.view(torch.int32).fill_(fill)
        return t if dtype is None else t.view(dtype)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    L = sparse_rx._capi.lib()
    arena = Arena(T.ARENA_BYTES)
    yield L, arena
    del arena.buf
    torch.cuda.empty_cache()


class Run:
    """One test's calls: each timed on its own (synchronised before and after), the status checked"""

    def __init__(self, L, name):
        import torch
        self.L, self.name, self.calls, self.t0 = L, name, [], time.perf_counter()
        self.stream = torch.cuda.current_stream().cuda_stream
        _KEEP.clear()
        torch.cuda.reset_peak_memory_stats()

    def call(self, entry, *args, expect=0):
        import torch
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc = getattr(self.L, entry)(*args)
        torch.cuda.synchronize()
        self.calls.append((time.perf_counter() - t, entry))
        assert rc == expect, f"{self.name}: {entry} returned {rc}: {self.L.srx_last_error().decode()}"
        return rc

    def timed(self, label, f):
        import torch
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        self.calls.append((time.perf_counter() - t, label))
        return out

    def done(self):
        import torch
        peak = torch.cuda.max_memory_allocated()
        assert peak <= T.CAP_BYTES, f"{self.name}: peak device memory {peak} above the cap of {T.CAP_BYTES}"
        slow = max(self.calls) if self.calls else (0.0, "-")
        fills = sum(t for t, n in self.calls if n.startswith("fill"))
        line = (f"{self.name}: wall {time.perf_counter() - self.t0:.3f} s, slowest call {slow[1]} {slow[0] * 1e3:.2f} ms, fills {fills * 1e3:.1f} ms, "
                f"library calls {sum(t for t, n in self.calls if n.startswith('srx_')) * 1e3:.1f} ms, peak memory {peak / 2 ** 30:.3f} GiB")
        print(line)
        path = os.environ.get("SRX_DENSE_SCALE_LOG")
        if path:
            with open(path, "a", encoding="utf-8") as fh:
                fh.write(line + "\n")


def _ptr(t):
    return None if t is None else t.data_ptr()


_KEEP = []  # every tensor _dev made for the running test: a pointer handed to the library must outlive the call, and a
            # temporary's block would be given to the next small allocation (an output filled with the garbage word, for one)


def _dev(a):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    _KEEP.append(t)
    return t


def _count_nonzero(t, chunk=1 << 27):
    """torch.count_nonzero of a large tensor in pieces: a device reduction, nothing downloaded, and the temporaries of one piece
    (torch widens before it sums) stay far below the memory cap"""
    import torch
    flat = t.reshape(-1)
    return sum(int(torch.count_nonzero(flat[i: i + chunk])) for i in range(0, flat.numel(), chunk))


def _outs(nq, k):
    """(doc, score, count) filled with the garbage word; the score tensor is int32 here and read as float32 bits"""
    import torch
    return tuple(torch.full((n,), GARBAGE, dtype=torch.int32, device=DEV) for n in (nq * k, nq * k, nq))


def _rows_of(outs, nq, k):
    d, s, n = (x.cpu().numpy() for x in outs)
    return d.reshape(nq, k), s.view(F).reshape(nq, k), n


def _workspace(arena, nbytes):
    """the workspace and its guard, all garbage"""
    assert nbytes > 0 and nbytes % 4 == 0, nbytes
    return arena.take(nbytes + 4 * T.GUARD_WORDS, fill=GARBAGE)


def _guard_intact(ws, nbytes, label):
    import torch
    g = ws[nbytes:].view(torch.int32).cpu().numpy()
    assert len(g) == T.GUARD_WORDS and (g == GARBAGE).all(), f"{label}: the words behind the workspace were written: {g[:8]}"


def _assert_rows(got, exp, label):
    d, s, n = got
    ed, es, en = exp
    assert np.array_equal(n, en), f"{label}: counts differ: {n.tolist()} != {en.tolist()}"
    assert np.array_equal(np.ascontiguousarray(s).view(np.uint32), np.ascontiguousarray(es).view(np.uint32)), f"{label}: scores differ"
    assert np.array_equal(d, ed), f"{label}: ids differ\n{d}\n{ed}"


def _ranked(scores, rows, k, base, allow=None):
    """the searches' contract on the planted rows alone: > 0 only, (score desc, doc asc), ids = base + row, padded -1 / 0"""
    s = np.asarray(scores, F) if allow is None else np.where(allow, np.asarray(scores, F), F(-1.0))
    d, sc, n = dense_topk_rows(s, k)
    ids = np.where(d >= 0, np.asarray(rows, np.int64)[np.maximum(d, 0)] + base, -1).astype(np.int32)
    return ids, sc, n


def _control_sets(P):
    """planted positions whose column 1 is positive: three of them, fewer than any k of the table"""
    return sorted({0, P // 2, P - 1})


def _candidates(rows, n_docs, base, nq):
    """cand_doc i32[nq, m], cand_count: every planted row (100 % of them) in another order per query, then ids outside the shard
    and -1; the counts cut rows 2 .. at the planted rows, at 3 and at 0"""
    rows = np.asarray(rows, np.int64)
    P = len(rows)
    out_of_range = [-1, base - 1, base + n_docs, T.MAX_ID + 1]
    cand = np.empty((nq, P + len(out_of_range)), np.int64)
    for q in range(nq):
        cand[q, :P] = np.roll(rows, q) + base
        cand[q, P:] = out_of_range
    cnt = np.array(([P + 4, P + 4, P, 3, 0] * nq)[:nq], np.int32)
    return cand.astype(np.int32), cnt


def _gather_scores(S, rows, cand, cnt, n_docs, base, pad=F(0.0)):
    """out[q][c] = S[q][position of the row] for live candidates, `pad` elsewhere (rescore_ref.live_candidates)"""
    pos = {int(r): j for j, r in enumerate(rows)}
    live, local = rescore_ref.live_candidates(cand, cnt, n_docs, base)
    out = np.full(cand.shape, pad, S.dtype)
    for q, c in zip(*np.nonzero(live)):
        out[q, c] = S[q, pos[int(local[q, c])]]
    return out


def _filter_rows(arena, case, rows):
    """Two filter rows written with torch, word by word: row 0 allows every doc but planted[1] and planted[-1], row 1 only
    planted[0], planted[2] and planted[-1].  Returns (bits tensor, allow bool[2, P])."""
    import torch
    words = T.filter_words(case.n_docs)
    assert filter_ref.words(case.n_docs) == words
    bits = arena.take(2 * words * 4, torch.int32).view(2, words)
    bits[0].fill_(-1)
    bits[1].zero_()
    P = len(rows)
    allow = np.zeros((2, P), bool)
    allow[0] = True
    allow[0, [1, P - 1]] = False
    allow[1, [0, 2, P - 1]] = True
    for r in (0, 1):
        want = {}
        for j in range(P):
            if allow[r, j] != (r == 0):  # the bits that differ from the row's fill
                want.setdefault(rows[j] >> 5, 0)
                want[rows[j] >> 5] |= 1 << (rows[j] & 31)
        for w, m in want.items():
            v = (0xFFFFFFFF ^ m) if r == 0 else m
            bits[r, w] = v - (1 << 32) if v >= 1 << 31 else v
    return bits, allow


def _filter_desc(bits, n_filters, q_filter):
    from sparse_rx import _capi
    return _capi.DocFilterDesc(bits=bits.data_ptr(), n_filters=n_filters, q_filter=_ptr(q_filter))


Q_FILTER = [0, 1, -1, 0, 1]


def _q_filter(nq):
    return np.array((Q_FILTER * -(-nq // len(Q_FILTER)))[:nq], np.int32)


def _allow_per_query(allow, nq):
    return np.stack([np.ones(allow.shape[1], bool) if _q_filter(nq)[q] < 0 else allow[_q_filter(nq)[q]] for q in range(nq)])


def _check_reference_shape(case, S, k):
    """what the issue asks of the planted scores: one query ranks more positive rows than k, one fewer, negative scores exist"""
    pos = (S > 0).sum(axis=1)
    assert pos[0] == S.shape[1] > k and 0 < pos[1] < k and pos[3] == 0 and (S[1] < 0).any(), (case.name, pos.tolist())


# ---- (a) (a') (b) (c): f32 and uint8 rows ------------------------------------------------------------------------------------------
def _float_world(case):
    """planted f32 rows and queries: column 0 is +50 everywhere (query 0 ranks every row), column 1 is +50 in three rows and -50
    in the others (query 1 ranks three and sees negative scores), query 3 ranks none; the last row repeats the first (a tie
    across the whole corpus)"""
    rows = case.planted()
    P = len(rows)
    rng = np.random.default_rng(len(case.name) + case.dim + P)
    R = rng.standard_normal((P, case.dim)).astype(F)
    R[:, 0] = 50
    R[:, 1] = -50
    R[_control_sets(P), 1] = 50
    R[P - 1] = R[0]
    Q = rng.standard_normal((case.nq, case.dim)).astype(F)
    Q[-1, 0] = abs(Q[-1, 0])  # the query of the second pass leans towards column 0: it ranks some rows
    Q[[0, 1, 3]] *= F(0.01)
    Q[0, 0], Q[1, 1], Q[3, 0] = 1, 1, -1
    Q[0, 1] = Q[1, 0] = Q[3, 1] = 0
    return rows, R, Q


def _u8_world(case):
    """the same construction in codes: code 255 de-quantizes to 255 s + min > 0, code 0 to min < 0"""
    rows = case.planted()
    P = len(rows)
    rng = np.random.default_rng(len(case.name) + case.dim + P)
    C = rng.integers(0, 256, (P, case.dim), dtype=np.uint8)
    C[:, 0] = 255
    C[:, 1] = 0
    C[_control_sets(P), 1] = 255
    sm = np.empty((P, 2), F)
    sm[:, 0] = F(0.01) + F(0.001) * (np.arange(P) % 4).astype(F)
    sm[:, 1] = F(-1.27)
    C[P - 1], sm[P - 1] = C[0], sm[0]
    Q = rng.standard_normal((case.nq, case.dim)).astype(F)
    Q[-1, 0] = abs(Q[-1, 0])
    Q[[0, 1, 3]] *= F(0.001)
    Q[0, 0], Q[1, 1], Q[3, 0] = 10, 10, -10
    Q[0, 1] = Q[1, 0] = Q[3, 1] = 0
    return rows, C, sm, Q


ROWS_CASES = ["a-f32-1024", "a-f32-768", "b-f32-1024", "c-u8-1024"]


@pytest.mark.parametrize("name", ROWS_CASES)
def test_rows_search_and_scorer_past_the_boundaries(gpu, name):
    import torch
    L, arena = gpu
    case = CASES[name]
    run = Run(L, name)
    arena.reset()
    n, dim, nq, k = case.n_docs, case.dim, case.nq, case.k
    u8 = case.kind == "u8"
    if u8:
        rows, R, sm, Q = _u8_world(case)
        S = dense_rows_scores(R, Q, scale_min=sm.reshape(-1))
        S_docs = np.stack([rescore_ref.lane_dot(R.astype(F) * sm[:, :1] + sm[:, 1:], Q[q]) for q in range(nq)])
    else:
        rows, R, Q = _float_world(case)
        S = dense_rows_scores(R, Q)
        S_docs = np.stack([rescore_ref.lane_dot(R, Q[q]) for q in range(nq)])
    assert np.array_equal(S.view(np.uint32), S_docs.view(np.uint32)), "the two restatements of the lane sum disagree"
    _check_reference_shape(case, S, k)
    corpus = arena.take(case.corpus_bytes(), torch.uint8 if u8 else torch.float32)
    run.timed("fill corpus", lambda: corpus.zero_())
    corpus = corpus.view(n, dim)
    scales = None
    if u8:
        scales = arena.take(8 * n, torch.float32, fill=0).view(n, 2)  # [2 d] scale, [2 d + 1] min: zeros for the zero rows
    dR = _dev(R)
    for j, r in enumerate(rows):  # one row at a time: plain slices, no index arithmetic of torch's at these sizes
        corpus[r].copy_(dR[j])
        if u8:
            scales[r].copy_(_dev(sm[j]))
    dQ = _dev(Q)
    ws_bytes = L.srx_dense_f32_workspace_bytes(nq, n, k)
    assert ws_bytes == case.workspace_bytes(), "restated srx_dense_f32_workspace_bytes drifted"
    ws = _workspace(arena, ws_bytes)
    bits, allow = _filter_rows(arena, case, rows)
    qf = _dev(_q_filter(nq))
    assert arena.off <= case.device_bytes() + 4096, "the table's byte column is below what the case takes"
    head = (0, _ptr(corpus)) + ((_ptr(scales),) if u8 else ()) + (n, dim, _ptr(dQ), nq, k)
    off = () if u8 else (ctypes.c_float(0.0),)
    # the plain search at the largest legal doc_base, and at 0
    for base in (case.doc_base_top, 0):
        outs = _outs(nq, k)
        run.call(case.entries[0], *head, base, *(_ptr(o) for o in outs), _ptr(ws), ws_bytes, run.stream, *off)
        _assert_rows(_rows_of(outs, nq, k), _ranked(S, rows, k, base), f"{name} {case.entries[0]} doc_base {base}")
        _guard_intact(ws, ws_bytes, name)
    # the filtered search: rows 0 / 1 / none per query
    base = case.doc_base_top
    desc = _filter_desc(bits, 2, qf)
    outs = _outs(nq, k)
    run.call(case.entries[1], *head, base, ctypes.byref(desc), *(_ptr(o) for o in outs), _ptr(ws), ws_bytes, run.stream, *off)
    _assert_rows(_rows_of(outs, nq, k), _ranked(S, rows, k, base, _allow_per_query(allow, nq)), f"{name} {case.entries[1]}")
    _guard_intact(ws, ws_bytes, name)
    # the scorer of given docs: every planted row, ids outside the shard, padding
    cand, cnt = _candidates(rows, n, base, nq)
    out = torch.full(cand.shape, GARBAGE, dtype=torch.int32, device=DEV)
    run.call(case.entries[2], *head[:-1], base, _ptr(_dev(cand)), _ptr(_dev(cnt)), cand.shape[1], _ptr(out), run.stream)
    exp = _gather_scores(S_docs, rows, cand, cnt, n, base)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32)), f"{name} {case.entries[2]}"
    run.done()


# ---- (i) filter rows past bit 2^32, then (c)'s filtered search through the last row -------------------------------------------------
def test_filter_rows_past_bit_2_32(gpu):
    import torch
    L, arena = gpu
    case = CASES["c-u8-1024"]
    n, n_filters = T.FILTER_CASE["n_docs"], T.FILTER_CASE["n_filters"]
    assert n == case.n_docs
    run = Run(L, "i-filter-rows")
    arena.reset()
    words = L.srx_filter_words(n)
    assert words == T.filter_words(n)
    bits = arena.take(n_filters * words * 4, torch.int32, fill=GARBAGE).view(n_filters, words)
    last = n_filters - 1
    run.call("srx_filter_fill", 0, _ptr(bits), n_filters, n, 0, run.stream)
    assert _count_nonzero(bits) == 0, "value 0: every word of every row is written"
    run.call("srx_filter_fill", 0, _ptr(bits), n_filters, n, 1, run.stream)
    tail = (1 << (n & 31)) - 1  # the last word with doc bits: the bits at or above n_docs are 0, the padding words too
    exp_full = np.zeros(words, np.uint32)
    exp_full[: n >> 5] = 0xFFFFFFFF
    exp_full[n >> 5] = tail
    assert bool((bits == _dev(exp_full.view(np.int32))[None, :]).all()), "value 1: some row differs from the full row"
    for r in (0, last - 1, last):
        assert np.array_equal(bits[r].cpu().numpy().view(np.uint32), exp_full), f"row {r} after the fill"
    # clear some docs of the last row and of its neighbour through the global ids of a doc_base at the top of the range
    rows = case.planted()
    base = case.doc_base_top
    cleared = {last: [rows[1], rows[-1], 5, 31, 32], last - 1: [rows[0], 7]}
    for r, docs in cleared.items():
        ids = _dev(np.array([d + base for d in docs] + [-1, base - 1, base + n, docs[0] + base], np.int32))  # ignored ids, a duplicate
        run.call("srx_filter_set_docs", 0, _ptr(bits[r]), n, base, _ptr(ids), len(ids), 0, run.stream)
    counts = torch.full((n_filters,), GARBAGE, dtype=torch.int32, device=DEV)
    run.call("srx_filter_count", 0, _ptr(bits), n_filters, n, _ptr(counts), run.stream)
    exp_counts = np.full(n_filters, n, np.int32)
    exp_counts[last], exp_counts[last - 1] = n - 5, n - 2
    assert np.array_equal(counts.cpu().numpy(), exp_counts)
    for r, docs in cleared.items():
        e = exp_full.copy()
        for d in docs:
            e[d >> 5] &= ~np.uint32(1 << (d & 31))
        assert np.array_equal(bits[r].cpu().numpy().view(np.uint32), e), f"row {r} after set_docs"
    assert bool((bits[: last - 1] == _dev(exp_full.view(np.int32))[None, :]).all()), "rows below the edited ones were written"
    # (c)'s filtered search with q_filter pointing at the last row
    _, R, sm, Q = _u8_world(case)
    S = dense_rows_scores(R, Q, scale_min=sm.reshape(-1))
    nq, k, dim = case.nq, case.k, case.dim
    corpus = arena.take(case.corpus_bytes(), torch.uint8)
    run.timed("fill corpus", lambda: corpus.zero_())
    corpus = corpus.view(n, dim)
    scales = arena.take(8 * n, torch.float32, fill=0).view(n, 2)
    dR = _dev(R)
    for j, r in enumerate(rows):
        corpus[r].copy_(dR[j])
        scales[r].copy_(_dev(sm[j]))
    ws_bytes = L.srx_dense_f32_workspace_bytes(nq, n, k)
    ws = _workspace(arena, ws_bytes)
    qf_host = np.array([last, last - 1, -1, last, last], np.int32)
    desc = _filter_desc(bits, n_filters, _dev(qf_host))
    allow = np.ones((nq, len(rows)), bool)
    for q in range(nq):
        for d in cleared.get(int(qf_host[q]), []):
            if d in rows:
                allow[q, rows.index(d)] = False
    outs = _outs(nq, k)
    dQ = _dev(Q)
    run.call("srx_dense_search_u8_filtered", 0, _ptr(corpus), _ptr(scales), n, dim, _ptr(dQ), nq, k, base, ctypes.byref(desc),
             *(_ptr(o) for o in outs), _ptr(ws), ws_bytes, run.stream)
    _assert_rows(_rows_of(outs, nq, k), _ranked(S, rows, k, base, allow), "u8 filtered through filter row 1024")
    _guard_intact(ws, ws_bytes, "i-filter-rows")
    run.done()


# ---- (d): INT8 rows, row-major and packed ------------------------------------------------------------------------------------------
def _i8_world(case, zero_col0=False):
    """planted int8 rows and queries, the construction of _float_world in codes.  zero_col0 (the plan cases): column 0 is left
    to the background, the controls sit in columns 1 and 2."""
    rows = case.planted()
    P = len(rows)
    c0 = 1 if zero_col0 else 0
    rng = np.random.default_rng(len(case.name) + case.dim + P)
    R = rng.integers(-20, 21, (P, case.dim), dtype=np.int8)
    R[:, c0] = 100
    R[:, c0 + 1] = -100
    R[_control_sets(P), c0 + 1] = 100
    cs = (F(0.5) + F(0.01) * np.arange(P)).astype(F)
    R[P - 1], cs[P - 1] = R[0], cs[0]
    Q = rng.integers(-127, 128, (case.nq, case.dim), dtype=np.int8)
    Q[[0, 1, 3]] = rng.integers(-1, 2, (3, case.dim), dtype=np.int8)
    Q[0, c0], Q[1, c0 + 1], Q[3, c0] = 127, 127, -127
    Q[0, c0 + 1] = Q[1, c0] = Q[3, c0 + 1] = 0
    qs = ((rng.random(case.nq) + 0.01) / 127).astype(F)
    return rows, R, cs, Q, qs


def _tile_groups(rows, per):
    g = {}
    for j, r in enumerate(rows):
        g.setdefault(r // per, []).append(j)
    return g


@pytest.mark.parametrize("name", ["d-i8-1024", "d-i8-768"])
def test_int8_rows_pack_and_scorer_past_the_boundaries(gpu, name):
    import torch
    L, arena = gpu
    case = CASES[name]
    run = Run(L, name)
    arena.reset()
    n, dim, nq, k = case.n_docs, case.dim, case.nq, case.k
    rows, R, cs, Q, qs = _i8_world(case)
    S = np_oracle.int8_similarities(Q, R, qs, cs)
    _check_reference_shape(case, S, k)
    corpus = arena.take(n * dim, torch.int8)
    run.timed("fill corpus", lambda: corpus.zero_())
    corpus = corpus.view(n, dim)
    packed_bytes = L.srx_dense_packed_bytes(n, dim)
    assert packed_bytes == -(-n // 32) * 32 * dim
    packed = arena.take(packed_bytes, torch.int8, fill=GARBAGE)  # the pack writes every byte, the zero rows of the last tile too
    scale = arena.take(4 * n, torch.float32, fill=0)
    dR = _dev(R)
    for j, r in enumerate(rows):
        corpus[r].copy_(dR[j])
    scale[_dev(np.array(rows, np.int64))] = _dev(cs)
    dQ, dqs = _dev(Q), _dev(qs)
    # srx_dense_pack_i8: the tiles that hold planted rows against the layout restatement, and nothing else non-zero anywhere
    run.call("srx_dense_pack_i8", 0, _ptr(corpus), n, dim, _ptr(packed), run.stream)
    tile_bytes = 32 * dim
    for t, members in _tile_groups(rows, 32).items():
        mini = np.zeros((32, dim), np.int8)
        for j in members:
            mini[rows[j] - 32 * t] = R[j]
        got = packed[t * tile_bytes: (t + 1) * tile_bytes].cpu().numpy()
        assert np.array_equal(got, rescore_ref.pack_i8(mini)), f"{name}: tile {t} of the packed corpus"
        for j in members:  # and the header's formula for every 16-byte piece of the row, in whole-corpus offsets
            offs = rescore_ref.packed_offsets(rows[j], dim)
            assert all(np.array_equal(packed[o: o + 16].cpu().numpy(), R[j, 16 * p: 16 * p + 16]) for p, o in enumerate(offs)), (name, rows[j])
    nz = run.timed("count_nonzero packed", lambda: _count_nonzero(packed))
    assert nz == int(np.count_nonzero(R)), f"{name}: {nz} non-zero bytes in the packed corpus, {np.count_nonzero(R)} planted"
    ws_bytes = L.srx_dense_workspace_bytes(nq, n, k)
    assert ws_bytes == case.workspace_bytes() == dense_ws(nq, n, k)["bytes"]
    ws = _workspace(arena, ws_bytes)
    assert arena.off <= case.device_bytes() + 4096
    for entry, store in (("srx_dense_search_i8", corpus), ("srx_dense_search_i8_packed", packed)):
        for base in (case.doc_base_top, 0):
            outs = _outs(nq, k)
            run.call(entry, 0, _ptr(store), _ptr(scale), n, dim, _ptr(dQ), _ptr(dqs), nq, k, base, *(_ptr(o) for o in outs), _ptr(ws), ws_bytes,
                     run.stream)
            _assert_rows(_rows_of(outs, nq, k), _ranked(S, rows, k, base), f"{name} {entry} doc_base {base}")
            _guard_intact(ws, ws_bytes, name)
    base = case.doc_base_top
    cand, cnt = _candidates(rows, n, base, nq)
    exp = _gather_scores(rescore_ref.i8_scores(R, cs, Q, qs, np.tile(np.arange(len(rows)), (nq, 1))), rows, cand, cnt, n, base)
    assert np.array_equal(_gather_scores(S, rows, cand, cnt, n, base).view(np.uint32), exp.view(np.uint32))
    for is_packed, store in ((0, corpus), (1, packed)):
        out = torch.full(cand.shape, GARBAGE, dtype=torch.int32, device=DEV)
        run.call("srx_dense_score_docs_i8", 0, _ptr(store), is_packed, _ptr(scale), n, dim, _ptr(dQ), _ptr(dqs), nq, base, _ptr(_dev(cand)),
                 _ptr(_dev(cnt)), cand.shape[1], _ptr(out), run.stream)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32)), f"{name} srx_dense_score_docs_i8 packed={is_packed}"
    run.done()


# ---- (j): the large-corpus branches of the INT8 pass plan ---------------------------------------------------------------------------
def _plan_id(name):
    c = CASES[name]
    return f"{name}-" + dense_plan_label(dense_plan(c.nq, c.n_docs, c.k, c.dim), c.k)


def _overflow_queries(case):
    """rows of the first pass that go through the score matrix: the last one, and every row a matrix boundary falls into"""
    return sorted({case.qb - 1} | {q for m in case.matrix for q, _ in T.matrix_cells(case, m)})


@pytest.mark.parametrize("name", [c.name for c in T.PLAN_CASES], ids=[_plan_id(c.name) for c in T.PLAN_CASES])
def test_int8_plan_large_corpus_branches(gpu, name):
    """QB 960, 256 and 32 with nq = QB + 1: two passes, the second of one query.  The plan picks the filtered path at these sizes;
    the matrix path is reached through its fallback: column 0 of EVERY doc is 1 (the only non-zero background), the queries
    named by _overflow_queries have q[0] = 127 and score every doc > 0 with one tie value, their candidate buffers overflow and
    their rows are ranked from the score matrix -- among them the last row of the pass, where q * ld + d is largest.  All
    other queries have q[0] = 0 and see a zero background.  An overflow query ranks the three planted rows above the tie, then
    the lowest doc ids of the background."""
    import torch
    L, arena = gpu
    case = CASES[name]
    run = Run(L, name)
    arena.reset()
    n, dim, nq, k, QB = case.n_docs, case.dim, case.nq, case.k, case.qb
    p = dense_plan(nq, n, k, dim)
    assert p["QB"] == QB and p["passes"] == 2 and p["path"] == "filtered", p
    ws_bytes = L.srx_dense_workspace_bytes(nq, n, k)
    w = dense_ws(nq, n, k)
    assert ws_bytes == w["bytes"] == case.workspace_bytes(), f"restated dense_ws drifted (nq={nq} n={n} k={k})"
    rows, R, cs, Q, qs = _i8_world(case, zero_col0=True)
    P = len(rows)
    R[:, 0] = 1
    cs[:] = 1  # corpus_scale is 1 everywhere, so the background ties exactly
    rng = np.random.default_rng(QB)
    Q[:, 0] = 0
    Q[QB] = Q[0]  # the second pass's only query: ranks every planted row
    Q[QB, 3:] = rng.integers(-1, 2, dim - 3)
    ovf_q = _overflow_queries(case)
    cell_of = {q: d for m in case.matrix for q, d in T.matrix_cells(case, m)}
    for q in ovf_q:
        Q[q] = 0
        Q[q, 0] = 127  # 127 in the background
        if q in cell_of:  # the two docs either side of the boundary cell of this row must be seen: the query leans on their columns
            two = R[rows.index(cell_of[q]) - 1: rows.index(cell_of[q]) + 1, 3:].astype(np.int64).sum(axis=0)
            Q[q, 3:] = 2 * np.sign(two)
            Q[q, 1] = -2  # column 1 is 100 in every planted row: the rows the query does not lean on fall below the background's tie
        else:             # 127 (1 + 100) in the three control rows, 127 (1 - 100) < 0 in the others
            Q[q, 2] = 127
            Q[q, 3:] = rng.integers(-1, 2, dim - 3)
    S = np_oracle.int8_similarities(Q, R, qs, cs)
    tie = np_oracle.int8_similarities(Q, np.eye(1, dim, dtype=np.int8), qs, np.ones(1, F))[:, 0]  # what a background doc scores
    assert (tie[ovf_q] > 0).all() and np.count_nonzero(tie) == len(ovf_q)
    normal = np.setdiff1d(np.arange(nq), ovf_q)
    assert min(ovf_q) > 3
    _check_reference_shape(case, S, k)
    in_round_1 = np.array(rows) < p["S1"]  # fewer than k planted rows in the sample and in the first round: both thresholds stay 0,
    assert in_round_1.sum() < k            # so every positive score of a query survives the filter
    assert (S[QB] > 0).sum() == P > k
    corpus = arena.take(n * dim, torch.int8)
    run.timed("fill corpus", lambda: corpus.zero_())
    corpus = corpus.view(n, dim)
    run.timed("fill column 0", lambda: corpus[:, 0].fill_(1))
    scale = arena.take(4 * n, torch.float32)
    scale.fill_(1.0)
    dR = _dev(R)
    for j, r in enumerate(rows):
        corpus[r].copy_(dR[j])
    nz = run.timed("count_nonzero corpus", lambda: _count_nonzero(corpus))
    assert nz == n - P + int(np.count_nonzero(R)), "the background column or the planted rows were not written as meant"
    ws = _workspace(arena, ws_bytes)
    assert arena.off <= case.device_bytes() + 4096
    dQ, dqs = _dev(Q), _dev(qs)
    # expected rows: the planted ranking; for an overflow query the planted rows above the tie, then the lowest background ids
    background = [d for d in range(k + P) if d not in set(rows)][:k]

    def expected(base, sel):
        ed, es, en = _ranked(S[sel], rows, k, base)
        for i, q in enumerate(sel):
            if q in ovf_q:
                top = sorted(((float(S[q, j]), rows[j]) for j in range(P) if S[q, j] > tie[q]), key=lambda t: (-t[0], t[1]))[:k]
                assert 0 < len(top) < k and not (S[q] == tie[q]).any(), "planted rows above the tie, then the background"
                if q in cell_of:
                    assert {cell_of[q] - 1, cell_of[q]} <= {r for _, r in top[:3]}, "the docs either side of the boundary cell lead the row"
                ed[i] = np.array([r for _, r in top] + background[: k - len(top)], np.int64) + base
                es[i] = [s for s, _ in top] + [tie[q]] * (k - len(top))
                en[i] = k
        return ed, es, en

    everyone = np.arange(nq)
    for base in (case.doc_base_top, 0):
        outs = _outs(nq, k)
        run.call("srx_dense_search_i8", 0, _ptr(corpus), _ptr(scale), n, dim, _ptr(dQ), _ptr(dqs), nq, k, base, *(_ptr(o) for o in outs), _ptr(ws),
                 ws_bytes, run.stream)
        _assert_rows(_rows_of(outs, nq, k), expected(base, everyone), f"{_plan_id(name)} doc_base {base}")
        _guard_intact(ws, ws_bytes, name)
    # the first pass alone: its overflow flags are still in the workspace (the second pass of the call above re-cleared them)
    outs = _outs(QB, k)
    run.call("srx_dense_search_i8", 0, _ptr(corpus), _ptr(scale), n, dim, _ptr(dQ), _ptr(dqs), QB, k, 0, *(_ptr(o) for o in outs), _ptr(ws), ws_bytes,
             run.stream)
    _assert_rows(_rows_of(outs, QB, k), expected(0, np.arange(QB)), f"{_plan_id(name)} first pass alone")
    w1 = dense_ws(QB, n, k)
    assert w1["bytes"] == ws_bytes and w1["qb"] == QB
    flags = ws[w1["ovf"]: w1["ovf"] + 4 * (QB + 1)].view(torch.int32).cpu().numpy()
    assert np.flatnonzero(flags[:QB]).tolist() == ovf_q and flags[QB] == 1, "the overflow queries, and only they, went through the score matrix"
    cnt = ws[w1["buf_cnt"]: w1["buf_cnt"] + 4 * QB * 32].view(torch.int32).cpu().numpy()[::32]
    assert np.array_equal(cnt[normal[normal < QB]], (S[normal[normal < QB]] > 0).sum(axis=1)), "survivor counts of the filtered path"
    _guard_intact(ws, ws_bytes, name)
    run.done()


# ---- (e): half rows in fragment order ----------------------------------------------------------------------------------------------
def _half_world(case):
    """small integers (exact in f16, bf16 and in the fp32 accumulator): the construction of _float_world with 8 / 64"""
    rows = case.planted()
    P = len(rows)
    rng = np.random.default_rng(len(case.name) + case.dim + P)
    R = rng.integers(-3, 4, (P, case.dim)).astype(np.int64)
    R[:, 0] = 8
    R[:, 1] = -8
    R[_control_sets(P), 1] = 8
    R[P - 1] = R[0]
    Q = rng.integers(-3, 4, (case.nq, case.dim)).astype(np.int64)
    Q[[0, 1, 3]] = rng.integers(-1, 2, (3, case.dim))
    Q[0, 0], Q[1, 1], Q[3, 0] = 64, 64, -64
    Q[0, 1] = Q[1, 0] = Q[3, 1] = 0
    for m in case.matrix:  # a row of the score matrix that holds a boundary cell ranks the docs either side of it first
        for q, d in T.matrix_cells(case, m):
            Q[q] = R[rows.index(d) - 1] + R[rows.index(d)]
    S = Q @ R.T
    assert np.abs(Q).dot(np.abs(R).T).max() < 2 ** 24
    for m in case.matrix:
        for q, d in T.matrix_cells(case, m):
            assert set(np.argsort(-S[q], kind="stable")[:3]) >= {rows.index(d) - 1, rows.index(d)}, (case.name, q, d)
    return rows, R, Q, S.astype(F)


def _plant_half(store_u16, rows, R, dtype, dim):
    """whole tiles of 32 rows through half_ref.pack"""
    tile_elems = 32 * dim
    for t, members in _tile_groups(rows, 32).items():
        mini = np.zeros((32, dim), F)
        for j in members:
            mini[rows[j] - 32 * t] = R[j]
        codes = half_ref.round_codes(mini, dtype).reshape(32, dim)
        store_u16[t * tile_elems: (t + 1) * tile_elems].copy_(_dev(half_ref.pack(codes).view(np.int16)))


@pytest.mark.parametrize("name", ["e-f16-1024", "e-bf16-1024", "e-f16-1024-8g", "e-f16-64-2p26"])
def test_half_search_and_scorer_past_the_boundaries(gpu, name):
    import torch
    L, arena = gpu
    case = CASES[name]
    run = Run(L, name)
    arena.reset()
    n, dim, nq, k, dtype = case.n_docs, case.dim, case.nq, case.k, case.kind
    rows, R, Q, S = _half_world(case)
    _check_reference_shape(case, S, k)
    nbytes = L.srx_dense_half_bytes(n, dim)
    assert nbytes == case.corpus_bytes() == half_ref.half_bytes(n, dim)
    store = arena.take(nbytes, torch.int16)
    run.timed("fill corpus", lambda: store.zero_())
    _plant_half(store, rows, R, dtype, dim)
    for r in (rows[0], rows[len(rows) // 2], rows[-1]):  # the header's formula in whole-corpus offsets, for three rows
        j = rows.index(r)
        for c in (0, 1, 9, dim - 1):
            o = half_ref.byte_offset(r, c, dim) // 2
            assert int(store[o]) == int(half_ref.round_codes(np.array([R[j, c]], F), dtype).view(np.int16)[0]), (name, r, c)
    ws_bytes = L.srx_dense_half_workspace_bytes(nq, n, k)
    assert ws_bytes == case.workspace_bytes(), "restated half_ws drifted"
    ws = _workspace(arena, ws_bytes)
    bits, allow = _filter_rows(arena, case, rows)
    qf = _dev(_q_filter(nq))
    assert arena.off <= case.device_bytes() + 4096
    dQ = _dev(Q.astype(F))
    ty = half_ref.TYPES[dtype]
    for base in (case.doc_base_top, 0):
        outs = _outs(nq, k)
        run.call("srx_dense_search_half", 0, ty, _ptr(store), n, dim, _ptr(dQ), nq, k, base, None, *(_ptr(o) for o in outs), _ptr(ws), ws_bytes,
                 run.stream, ctypes.c_float(0.0))
        _assert_rows(_rows_of(outs, nq, k), _ranked(S, rows, k, base), f"{name} srx_dense_search_half doc_base {base}")
        _guard_intact(ws, ws_bytes, name)
    base = case.doc_base_top
    desc = _filter_desc(bits, 2, qf)
    outs = _outs(nq, k)
    run.call("srx_dense_search_half", 0, ty, _ptr(store), n, dim, _ptr(dQ), nq, k, base, ctypes.byref(desc), *(_ptr(o) for o in outs), _ptr(ws),
             ws_bytes, run.stream, ctypes.c_float(0.0))
    _assert_rows(_rows_of(outs, nq, k), _ranked(S, rows, k, base, _allow_per_query(allow, nq)), f"{name} srx_dense_search_half filtered")
    _guard_intact(ws, ws_bytes, name)
    cand, cnt = _candidates(rows, n, base, nq)
    out = torch.full(cand.shape, GARBAGE, dtype=torch.int32, device=DEV)
    run.call("srx_dense_score_docs_half", 0, ty, _ptr(store), n, dim, _ptr(dQ), nq, base, _ptr(_dev(cand)), _ptr(_dev(cnt)), cand.shape[1], _ptr(out),
             run.stream)
    exp = _gather_scores(S, rows, cand, cnt, n, base)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32)), f"{name} srx_dense_score_docs_half"
    run.done()


# ---- (f): binary codes -------------------------------------------------------------------------------------------------------------
def test_binary_search_and_distances_past_byte_2_32(gpu):
    """No > 0 rule: the zero rows tie at popcount(q) and the tail of the m nearest is the lowest doc ids at that distance.
    Expected rows come from binary_ref.search on the planted rows plus the first m + P other docs (all-zero codes): no other
    background doc can be among the m nearest.  Query 1 is all zeros (every background doc at distance 0), query 2 all ones."""
    import torch
    L, arena = gpu
    case = CASES["f-binary-1024"]
    run = Run(L, case.name)
    arena.reset()
    n, dim, nq, m = case.n_docs, case.dim, case.nq, case.k
    W = dim // 32
    rows = case.planted()
    P = len(rows)
    rng = np.random.default_rng(P + dim)
    q_bits = rng.integers(0, 1 << 32, (nq, W), dtype=np.uint64).astype(np.uint32)
    q_bits[1], q_bits[2] = 0, 0xFFFFFFFF
    Rb = rng.integers(0, 1 << 32, (P, W), dtype=np.uint64).astype(np.uint32)
    Rb[1] = q_bits[0]
    Rb[1, 7] ^= np.uint32(1 << 9)           # one bit from query 0
    Rb[2] = q_bits[0]                       # distance 0
    Rb[3] = ~q_bits[0]                      # the complement: distance 1024
    Rb[P - 1] = Rb[0]                       # a tie across the whole corpus
    small = sorted(set(rows) | set([d for d in range(m + 2 * P) if d not in set(rows)][: m + P]))
    small_bits = np.zeros((len(small), W), np.uint32)
    for j, r in enumerate(rows):
        small_bits[small.index(r)] = Rb[j]
    ids = np.array(small, np.int64)

    def expected(base, masks=None, q_filter=None):
        d, dist, cnt = binary_ref.search(q_bits, small_bits, m, 0, masks, q_filter)
        return np.where(d >= 0, ids[np.maximum(d, 0)] + base, -1).astype(np.int32), dist, cnt

    nbytes = L.srx_binary_bytes(n, dim, 1)
    assert nbytes == case.corpus_bytes()
    store = arena.take(nbytes, torch.int32)
    run.timed("fill corpus", lambda: store.zero_())
    tile_words = 64 * W
    for t, members in _tile_groups(rows, 64).items():
        mini = np.zeros((64, W), np.uint32)
        for j in members:
            mini[rows[j] - 64 * t] = Rb[j]
        store[t * tile_words: (t + 1) * tile_words].copy_(_dev(binary_ref.tile(mini).view(np.int32)))
    for j in (0, P // 2, P - 1):  # the header's formula in whole-corpus indices
        for wd in (0, 5, W - 1):
            assert int(store[binary_ref.tiled_index(rows[j], wd, W)]) == int(Rb[j, wd:wd + 1].view(np.int32)[0]), (rows[j], wd)
    ws_bytes = L.srx_binary_workspace_bytes(nq, n, m)
    assert ws_bytes == case.workspace_bytes(), "the header's workspace formula drifted"
    ws = _workspace(arena, ws_bytes)
    # filter rows: row 0 removes two planted rows and the background docs 1 and 2; row 1 allows three planted rows and docs 5, 7
    words = T.filter_words(n)
    fbits = arena.take(2 * words * 4, torch.int32).view(2, words)
    fbits[0].fill_(-1)
    fbits[1].zero_()
    masks = np.zeros((2, len(small)), bool)
    masks[0] = True
    for d in (rows[1], rows[-1], 1, 2):
        masks[0, small.index(d)] = False
    for d in (rows[0], rows[2], rows[-1], 5, 7):
        masks[1, small.index(d)] = True
    assert not {1, 2, 5, 7} & set(rows)
    for r in (0, 1):
        want = {}
        for i, d in enumerate(small):
            if masks[r, i] != (r == 0):
                want[d >> 5] = want.get(d >> 5, 0) | (1 << (d & 31))
        for wd, mask in want.items():
            v = (0xFFFFFFFF ^ mask) if r == 0 else mask
            fbits[r, wd] = v - (1 << 32) if v >= 1 << 31 else v
    assert arena.off <= case.device_bytes() + 4096
    dq = _dev(q_bits.view(np.int32))
    for base in (case.doc_base_top, 0):
        outs = _outs(nq, m)
        run.call("srx_binary_search", 0, _ptr(store), n, dim, _ptr(dq), nq, m, base, None, *(_ptr(o) for o in outs), _ptr(ws), ws_bytes, run.stream)
        d, dist, cnt = (x.cpu().numpy() for x in outs)
        ed, edist, ecnt = expected(base)
        assert np.array_equal(cnt, ecnt) and np.array_equal(dist.reshape(nq, m), edist) and np.array_equal(d.reshape(nq, m), ed), (base, d, ed)
        _guard_intact(ws, ws_bytes, case.name)
    base = case.doc_base_top
    q_filter = np.array([0, 1, -1], np.int32)
    desc = _filter_desc(fbits, 2, _dev(q_filter))
    outs = _outs(nq, m)
    run.call("srx_binary_search", 0, _ptr(store), n, dim, _ptr(dq), nq, m, base, ctypes.byref(desc), *(_ptr(o) for o in outs), _ptr(ws), ws_bytes,
             run.stream)
    d, dist, cnt = (x.cpu().numpy() for x in outs)
    ed, edist, ecnt = expected(base, masks, q_filter)
    assert ecnt[1] == 5 < m, "filter row 1 allows fewer docs than m: the row is padded -1 / -1"
    assert np.array_equal(cnt, ecnt) and np.array_equal(dist.reshape(nq, m), edist) and np.array_equal(d.reshape(nq, m), ed), (d, ed)
    _guard_intact(ws, ws_bytes, case.name)
    cand, ccnt = _candidates(rows, n, base, nq)
    out = torch.full(cand.shape, GARBAGE, dtype=torch.int32, device=DEV)
    run.call("srx_binary_dist_docs", 0, _ptr(store), n, dim, _ptr(dq), nq, base, _ptr(_dev(cand)), _ptr(_dev(ccnt)), cand.shape[1], _ptr(out), run.stream)
    exp = _gather_scores(binary_ref.distances(q_bits, Rb), rows, cand, ccnt, n, base, pad=np.int32(-1))
    assert np.array_equal(out.cpu().numpy(), exp), "srx_binary_dist_docs"
    run.done()


# ---- (g): MaxSim over token rows past byte 2^32 -------------------------------------------------------------------------------------
def test_maxsim_token_rows_past_byte_2_32(gpu):
    """Docs own 50 token rows each; the candidates are the docs whose token ranges lie below, across and above bytes 2^31 and
    2^32 of the store, the first doc and the last two (the last one shorter, ending inside the last tile)."""
    import torch
    L, arena = gpu
    case = CASES["g-tokens-128"]
    run = Run(L, case.name)
    arena.reset()
    n_tok, dim, nq, k, per = case.n_docs, case.dim, case.nq, case.k, 50
    n_docs = -(-n_tok // per)
    ptr = np.minimum(np.arange(n_docs + 1, dtype=np.int64) * per, n_tok)
    assert ptr[-1] == n_tok <= (1 << 31) - 2 and 0 < ptr[-1] - ptr[-2] < per
    docs = [0, n_docs - 2, n_docs - 1]
    for B in (T.B31, T.B32):
        t = B // case.row_bytes  # the first token row at or above the boundary
        d = t // per
        assert ptr[d] < t < ptr[d + 1], "a doc lies across the boundary"
        docs += [d - 1, d, d + 1]
    docs = sorted(set(docs))  # the doc above byte 2^32 is the last doc
    rng = np.random.default_rng(n_docs)
    tok_rows, tok_vals = [], []
    for d in docs:
        for r in range(int(ptr[d]), int(ptr[d + 1])):
            tok_rows.append(r)
            tok_vals.append(rng.integers(-3, 4, dim))
    TV = np.array(tok_vals, np.int64)
    tq = 33
    Q = rng.integers(-3, 4, (nq, tq, dim)).astype(np.int64)
    q_cnt = np.array([tq, 20, 0], np.int32)
    store = arena.take(L.srx_dense_half_bytes(n_tok, dim), torch.int16)
    assert store.numel() * 2 == case.corpus_bytes()
    run.timed("fill corpus", lambda: store.zero_())
    _plant_half(store, tok_rows, TV, "f16", dim)
    dptr = _dev(ptr.astype(np.int32))
    first = {d: tok_rows.index(int(ptr[d])) for d in docs}

    def pair(q, d):
        live = late_ref.live_tokens(q_cnt[q], tq)
        if live == 0:
            return F(0.0)
        sim = (Q[q, :live] @ TV[first[d]: first[d] + int(ptr[d + 1] - ptr[d])].T).astype(F)
        return late_ref.score_from_sim(sim, live)

    base = T.MAX_ID - n_docs
    m = len(docs) + 3
    cand = np.empty((nq, m), np.int64)
    for q in range(nq):
        cand[q] = list(np.roll(np.array(docs), q) + base) + [-1, base - 1, base + n_docs]
    cand = cand.astype(np.int32)
    ccnt = np.array([m, len(docs), m], np.int32)
    exp = np.zeros((nq, m), F)
    live = np.zeros((nq, m), bool)
    for q in range(nq):
        live[q] = late_ref.live_positions(cand[q], ccnt[q], base, n_docs)
        for c in np.flatnonzero(live[q]):
            exp[q, c] = pair(q, int(cand[q, c]) - base)
    ws_bytes = L.srx_maxsim_workspace_bytes(nq, tq, dim, m)
    ws = _workspace(arena, ws_bytes)
    dQ, dqc, dcand, dccnt = _dev(Q.astype(F)), _dev(q_cnt), _dev(cand), _dev(ccnt)
    out = torch.full((nq, m), GARBAGE, dtype=torch.int32, device=DEV)
    head = (0, half_ref.TYPES["f16"], _ptr(store), n_tok, dim, _ptr(dptr), n_docs, base, _ptr(dQ), _ptr(dqc), nq, tq, _ptr(dcand), _ptr(dccnt), m)
    run.call("srx_maxsim_score_docs_half", *head, _ptr(out), _ptr(ws), ws_bytes, run.stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32)), (out.cpu().numpy().view(F), exp)
    _guard_intact(ws, ws_bytes, case.name)
    outs = _outs(nq, k)
    run.call("srx_maxsim_rerank_half", *head, k, *(_ptr(o) for o in outs), _ptr(ws), ws_bytes, run.stream)
    ed, es, en = np.full((nq, k), -1, np.int32), np.zeros((nq, k), F), np.zeros(nq, np.int32)
    for q in range(nq):
        ed[q], es[q], en[q] = late_ref.rank(cand[q], exp[q], live[q], k)
    _assert_rows(_rows_of(outs, nq, k), (ed, es, en), "srx_maxsim_rerank_half")
    _guard_intact(ws, ws_bytes, case.name)
    run.done()


# ---- (h): converters whose chunk lies across byte 2^32 of the whole-corpus output ----------------------------------------------------
@pytest.mark.parametrize("conv", T.CONVERT_CASES, ids=[f"{c[1]}-{c[2]}" for c in T.CONVERT_CASES])
def test_converters_write_across_byte_2_32(gpu, conv):
    """The output buffer is the arena (not filled outside the span that is looked at): the chunk's bytes equal the restatement,
    the 64 tiles before and after it still hold the garbage word, the scale entries next to the chunk's too."""
    import torch
    L, arena = gpu
    entry, kind, dim, tile, n_rows = conv
    run = Run(L, f"h-{kind}-{dim}")
    arena.reset()
    row0, n_total, row_bytes, lo, hi = T.convert_geometry(kind, dim, tile, n_rows)
    guard = T.CONVERT_GUARD_TILES * max(tile, 1) * row_bytes
    out = arena.take(-(-n_total // max(tile, 1)) * max(tile, 1) * row_bytes)
    span = out[lo - guard: hi + guard]
    span.view(torch.int32).fill_(GARBAGE)
    E = quant_ref.make_rows(dim + n_rows, n_rows, dim, degenerate=False) if kind in ("i8-packed", "i8-rows", "u8-rows") else None
    rng = np.random.default_rng(dim)
    if kind.startswith("i8") or kind == "u8-rows":
        n_scale = n_total if kind.startswith("i8") else 2 * n_total
        scale = arena.take(4 * n_scale, torch.float32, fill=GARBAGE)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        dE = _dev(E)
        if kind.startswith("i8"):
            packed = int(kind == "i8-packed")
            run.call(entry, 0, _ptr(dE), dim, n_rows, dim, dim, row0, n_total, packed, _ptr(out), _ptr(scale), _ptr(flag), run.stream)
            codes, sc, fl = quant_ref.i8_rows(E, dim)
            exp = rescore_ref.pack_i8(codes) if packed else codes.reshape(-1)
            exp_scale = {row0: sc}
        else:
            run.call(entry, 0, _ptr(dE), dim, n_rows, dim, dim, row0, n_total, _ptr(out), _ptr(scale), _ptr(flag), run.stream)
            codes, sm, fl = quant_ref.u8_rows(E, dim)
            exp = codes.reshape(-1)
            exp_scale = {row0: sm[:n_rows], n_total + row0: sm[n_rows:]}
        assert int(flag) == fl
        got_scale = scale.cpu().numpy()
        keep = np.ones(n_scale, bool)
        for at, vals in exp_scale.items():
            assert quant_ref.same_bits(got_scale[at: at + n_rows], vals), f"{kind}: scales at {at}"
            keep[at: at + n_rows] = False
        assert (got_scale[keep].view(np.int32) == GARBAGE).all(), f"{kind}: a scale outside the chunk was written"
    elif kind in ("f16", "bf16"):
        E = (rng.standard_normal((n_rows, dim)) * 10.0 ** rng.uniform(-6, 4, (n_rows, 1))).astype(F)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        run.call(entry, 0, half_ref.TYPES[kind], _ptr(_dev(E)), dim, n_rows, dim, dim, row0, n_total, _ptr(out), _ptr(flag), run.stream)
        codes, fl = half_ref.convert(E, kind, dim)
        assert int(flag) == fl
        exp = half_ref.pack(codes).view(np.uint8)
    else:
        E = rng.standard_normal((n_rows, dim)).astype(F)
        center = (rng.standard_normal(dim) * 0.1).astype(F)
        run.call(entry, 0, _ptr(_dev(E)), dim, n_rows, dim, dim, row0, n_total, _ptr(_dev(center)), 1, _ptr(out), run.stream)
        exp = binary_ref.tile(binary_ref.encode(E, center, dim)).view(np.uint8)
    got = span.cpu().numpy()
    assert len(exp.reshape(-1).view(np.uint8)) == hi - lo
    assert np.array_equal(got[guard: guard + hi - lo], exp.reshape(-1).view(np.uint8)), f"{kind} dim {dim}: the chunk's output"
    assert (got[:guard].view(np.int32) == GARBAGE).all() and (got[guard + hi - lo:].view(np.int32) == GARBAGE).all(), f"{kind}: written outside the chunk"
    run.done()
