"""The sparse kernels past 2^31 / 2^32 bytes, words and padded positions of the posting arrays and past 2^30 / 2^31 entries of the
skip table, on the device.

Every case is a row of tests/sparse_scale.py.  The index lives in ONE zero-filled device arena (allocated once for the module
at the size of the largest case, never a host array); only the planted terms' blocks, skip rows, idf and term_bound entries and
the sentinel pad hold data, written in the stored form through parity.np_build_blocks / np_compact_blocks.  No query names a
filler term (tests/test_sparse_scale_cpu.py proves it), so the expected rows are the oracle's on the planted postings alone.
Calls go through the C ABI with the test's own buffers; outputs and workspaces are pre-filled with 0x7F7F7F7F, the workspace
is exactly srx_search_workspace_bytes long and the 64 words behind it must still hold the garbage word.  Every comparison is
exact.  The main batch of every case runs with doc_base + n_docs == 2^31 - 2.  Which tier served what is read back from the
workspace (parity.decode_routes) and compared with the restated hand-over rules.

Wall times and peak memory of every test go to the file SRX_SPARSE_SCALE_LOG names, if it is set (profiles/sparse_scale_tests.log
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

import build_ref  # noqa: E402
import filter_ref  # noqa: E402
import parity  # noqa: E402
import score_ref  # noqa: E402
import sparse_scale as T  # noqa: E402
import terms_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
GARBAGE = T.GARBAGE
K = T.K
CASES = {c.name: c for c in T.CASES}
# alternative paths over the same index, same rows: tier 2 alone; no term bounds; no flat tiles and no wave-level dense tiles
# (the packed path); the masked and the general form of the wave-level dense tiles; the block merge kernel
DEBUGS = (8, 16, 128 | 2048, 4096, 8192, 256)


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
    arena = Arena(T.arena_bytes())
    yield L, arena
    del arena.buf
    torch.cuda.empty_cache()


_KEEP = []  # every tensor _dev made for the running test: a pointer handed to the library must outlive the call


class Run:
    """One test's calls: each timed on its own (synchronised before and after), the status checked"""

    def __init__(self, L, name):
        import torch
        self.L, self.name, self.calls, self.t0 = L, name, [], time.perf_counter()
        self.stream = torch.cuda.current_stream().cuda_stream
        _KEEP.clear()
        torch.cuda.reset_peak_memory_stats()

    def call(self, entry, *args):
        import torch
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc = getattr(self.L, entry)(*args)
        torch.cuda.synchronize()
        self.calls.append((time.perf_counter() - t, entry))
        assert rc == 0, f"{self.name}: {entry} returned {rc}: {self.L.srx_last_error().decode()}"

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
                f"library calls {sum(t for t, n in self.calls if n.startswith('srx_')) * 1e3:.1f} ms in {sum(n.startswith('srx_') for _, n in self.calls)}, "
                f"peak memory {peak / 2 ** 30:.3f} GiB")
        print(line)
        path = os.environ.get("SRX_SPARSE_SCALE_LOG")
        if path:
            with open(path, "a", encoding="utf-8") as fh:
                fh.write(line + "\n")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(a):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    _KEEP.append(t)
    return t


def _count_nonzero(t, chunk=1 << 27):
    """torch.count_nonzero of a large tensor in pieces: a device reduction, nothing downloaded"""
    import torch
    flat = t.reshape(-1)
    return sum(int(torch.count_nonzero(flat[i: i + chunk])) for i in range(0, flat.numel(), chunk))


def _outs(nq, k):
    import torch
    return tuple(torch.full((n,), GARBAGE, dtype=torch.int32, device=DEV) for n in (nq * k, nq * k, nq))


def _rows_of(outs, nq, k):
    d, s, n = (x.cpu().numpy() for x in outs)
    return d.reshape(nq, k), s.view(F).reshape(nq, k), n


def _assert_rows(got, exp, label):
    d, s, n = got
    ed, es, en = exp
    assert np.array_equal(n, en), f"{label}: counts differ: {n.tolist()} != {en.tolist()}"
    assert np.array_equal(np.ascontiguousarray(s).view(np.uint32), np.ascontiguousarray(es).view(np.uint32)), f"{label}: scores differ\n{s}\n{es}"
    assert np.array_equal(d, ed), f"{label}: ids differ\n{d}\n{ed}"


def _guard_intact(ws, nbytes, label):
    import torch
    g = ws[nbytes:].view(torch.int32).cpu().numpy()
    assert len(g) == T.GUARD_WORDS and (g == GARBAGE).all(), f"{label}: the words behind the workspace were written: {g[:8]}"


# ---- the index of a case in the arena -----------------------------------------------------------------------------------------------
class World:
    """the planted index on the device, its descriptors and what the oracle says of its queries"""


def _plant(run, arena, lay):
    import torch
    from sparse_rx import _capi
    c = lay.case
    w = World()
    w.lay, w.case = lay, c
    w.copies = {}
    for copy in c.copies:
        words = c.words(copy)
        t = arena.take(lay.posting_bytes(copy), torch.int32)
        run.timed(f"fill {copy}", lambda: t.zero_())
        for p in lay.planted:
            if p["extent"]:
                t[p["ptr"] // 4 * words: (p["ptr"] + p["extent"]) // 4 * words].copy_(_dev(lay.blocks_of(p["small"], copy).reshape(-1)))
        t[lay.n_blocks * words:].copy_(_dev(lay.pad_blocks(copy).reshape(-1)))
        w.copies[copy] = t
    w.skip = arena.take(lay.vocab * c.row * 4, torch.int32)
    run.timed("fill tile_skip", lambda: w.skip.zero_())
    w.idf = arena.take(lay.vocab * 4, torch.float32, fill=0)
    w.bound = arena.take(lay.vocab * 16, torch.float32, fill=0)
    tb = lay.term_bound()
    for p in lay.planted:
        t = p["term"]
        w.skip[t * c.row: (t + 1) * c.row].copy_(_dev(lay.skip_row(p["small"])))
        w.bound[4 * t: 4 * t + 4].copy_(_dev(tb[p["small"]]))
    w.idf[_dev(np.array([p["term"] for p in lay.planted], np.int64))] = _dev(lay.idf_small)
    w.term_ptr = _dev(lay.term_ptr)
    assert arena.off <= lay.device_bytes(), "the table's byte column is below what the case takes"
    nnz = len(lay.csr[1])

    def desc(doc_base, copies=c.copies):
        return _capi.IndexDesc(device=0, val_type=T.VAL_TYPE[c.val], n_docs=c.n_docs, vocab=lay.vocab, nnz=nnz, n_blocks=lay.n_blocks,
                               doc_base=doc_base, tile_log2=c.tile_log2, n_tiles=c.n_tiles, unit_tiles=c.unit_tiles, reserved0=0,
                               term_ptr=_ptr(w.term_ptr), post=_ptr(w.copies["post"]) if "post" in copies else None, tile_skip=_ptr(w.skip),
                               idf=_ptr(w.idf), term_bound=_ptr(w.bound), post16=_ptr(w.copies["post16"]) if "post16" in copies else None)

    w.desc = desc
    w.q = tuple(_dev(x) for x in lay.queries)
    w.nq = len(lay.queries[0]) - 1
    w.full = T.full_scores(lay.csr, lay.idf_small, lay.queries_small, c.n_docs)
    return w


class Index:
    """an srx_index handle over a descriptor of the world, destroyed with the test"""

    def __init__(self, run, w, doc_base):
        self.run, self.w, self.base = run, w, doc_base
        self.d = w.desc(doc_base)
        self.h = ctypes.c_void_p()
        run.call("srx_index_create", ctypes.byref(self.d), ctypes.byref(self.h))

    def opts(self, target, debug):
        from sparse_rx import _capi
        o = _capi.SearchOpts(supertile_log2=0, target_blocks=target, profile=0, reserved=debug, unit_tiles=0)
        self.run.call("srx_index_set_opts", self.h, ctypes.byref(o))

    def close(self):
        self.run.L.srx_index_destroy(self.h)


def _expected_routes(w, p, debug):
    """(bits bool[items, n_super], the set of items on tier 2's worklist) by the restated rules"""
    lay, c = w.lay, w.case
    bits = np.zeros((p["items"], p["n_super"]), bool)
    if not T.tier1_serves(lay) or debug & 8:
        return bits, set(range(p["items"]))  # every query has terms: every item is tier 2's, no flag
    r = parity.tier1_routes(*lay.csr, np.ones(c.n_docs, F), lay.idf_small, lay.queries_small, c.tile_log2, c.unit_tiles, K, p,
                            term_bound=not (debug & 16), mode="dot", val_dtype=c.val)
    assert not r["may"].any() and not r["all_t2"].any()
    return r["must_flag"], set(np.flatnonzero(r["must_flag"].any(axis=1)).tolist())


def _search(run, arena, ix, entry, k, extra=(), packed=False, routes=None):
    """one search with a workspace of exactly the library's size (+ the guard), everything pre-filled with the garbage word"""
    import torch
    w, L = ix.w, run.L
    nq = w.nq
    ws_bytes = L.srx_search_workspace_bytes(ix.h, nq, k)
    mark = arena.off
    ws = arena.take(ws_bytes + 4 * T.GUARD_WORDS, fill=GARBAGE)
    if packed:
        out = torch.full((nq, 2 * k + 1), GARBAGE, dtype=torch.int32, device=DEV)
        run.call(entry, ix.h, *(_ptr(x) for x in w.q), nq, k, *extra, _ptr(out), _ptr(ws), ws_bytes, run.stream)
        rows = out.cpu().numpy()
        got = (rows[:, :k].copy(), rows[:, k:2 * k].copy().view(F), rows[:, 2 * k].copy())
    else:
        outs = _outs(nq, k)
        run.call(entry, ix.h, *(_ptr(x) for x in w.q), nq, k, *extra, *(_ptr(o) for o in outs), _ptr(ws), ws_bytes, run.stream)
        got = _rows_of(outs, nq, k)
    _guard_intact(ws, ws_bytes, f"{run.name} {entry}")
    if routes is not None:
        target, debug = routes
        p = parity.plan(w.case.n_tiles, w.case.unit_tiles, nq, k, target)
        assert parity.plan_workspace_bytes(p, nq, k) == ws_bytes, "restated planner drifted from make_plan"
        bits, work, n = parity.decode_routes(ws[:ws_bytes].cpu().numpy(), p, nq, k)
        exp_bits, exp_work = _expected_routes(w, p, debug)
        assert not bits[:, p["n_super"]:].any(), f"{run.name}: flag bits at or beyond n_super"
        assert np.array_equal(bits[:, : p["n_super"]], exp_bits), (
            f"{run.name} target {target} debug {debug}: flagged (item, unit) {np.argwhere(bits).tolist()[:12]}, written for {np.argwhere(exp_bits).tolist()[:12]}")
        assert len(work) == len(set(work)) and set(work) == exp_work, f"{run.name} target {target} debug {debug}: worklist {sorted(work)[:16]}"
    arena.off = mark
    return got


def _term(lay, group, local):
    """the real id of local term `local` of the group-th group"""
    return [p for p in lay.planted if p["group"] == group][local]


def _constraints(lay):
    """three filter rows over planted terms (real ids for the device, small ids for the restatement): docs with the long term of
    the first A group; docs with B's second term or H's second term; docs without H's first term and without term 0"""
    kinds = [g[0] for g in lay.case.groups]
    a, b, h = kinds.index("A"), kinds.index("B"), kinds.index("H")
    lists = {"all": [[_term(lay, a, 1)], [], []], "any": [[], [_term(lay, b, 2), _term(lay, h, 2)], []], "none": [[], [], [_term(lay, h, 1), _term(lay, 0, 0)]]}
    return ({k: [[p["term"] for p in row] for row in v] for k, v in lists.items()}, {k: [[p["small"] for p in row] for row in v] for k, v in lists.items()})


def _csr_lists(rows):
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return _dev(ptr), _dev(np.array([t for r in rows for t in r] + [0], np.int32))  # one spare element: never an empty allocation


@pytest.mark.parametrize("name", list(CASES))
def test_searches_past_the_boundaries(gpu, name):
    import torch
    from sparse_rx import _capi
    L, arena = gpu
    case = CASES[name]
    lay = T.build(case)
    run = Run(L, name)
    arena.reset()
    w = _plant(run, arena, lay)
    nq, base = w.nq, case.doc_base_top
    exp = T.ranked_rows(w.full, K, base)
    assert exp[2].min() >= 1 and exp[0].max() == (1 << 31) - 3
    serves = T.tier1_serves(lay)
    assert serves == (name in ("p-f32-both", "p-f16-compact", "p-f16-both", "s-lt30"))
    top = Index(run, w, base)
    # the plain search at the largest legal doc_base: one item per query, then the default plan (one item per unit)
    for target in (nq, 0):
        top.opts(target, 0)
        _assert_rows(_search(run, arena, top, "srx_search", K, routes=(target, 0)), exp, f"{name} srx_search target {target}")
    _assert_rows(_search(run, arena, top, "srx_search_packed", K, packed=True, routes=(0, 0)), exp, f"{name} srx_search_packed")
    # the alternative paths, at doc_base 0
    zero = Index(run, w, 0)
    exp0 = T.ranked_rows(w.full, K, 0)
    for debug in DEBUGS:
        target = 0 if debug == 256 else nq  # the merge kernels only run for split queries
        zero.opts(target, debug)
        _assert_rows(_search(run, arena, zero, "srx_search", K, routes=(target, debug) if debug in (8, 16) else None), exp0, f"{name} srx_search debug {debug}")
    zero.close()
    # search-after: the page behind each query's last row
    top.opts(nq, 0)
    last = np.maximum(exp[2] - 1, 0)
    after = (exp[0][np.arange(nq), last].copy(), exp[1][np.arange(nq), last].copy())
    exp_after = T.ranked_rows(w.full, K, base, after=after)
    assert exp_after[2].max() == K and exp_after[2].min() == 0, "some query has a full second page, some has none"
    ad, as_ = _dev(after[0]), _dev(after[1])
    _assert_rows(_search(run, arena, top, "srx_search_after", K, extra=(_ptr(ad), _ptr(as_))), exp_after, f"{name} srx_search_after")
    _assert_rows(_search(run, arena, top, "srx_search_after_packed", K, extra=(_ptr(ad), _ptr(as_)), packed=True), exp_after, f"{name} srx_search_after_packed")
    # srx_filter_from_terms over planted terms, from every copy the case carries, against the restatement
    big, small = _constraints(lay)
    masks = terms_ref.term_masks(lay.csr[0], lay.csr[1], case.n_docs, all=small["all"], any=small["any"], none=small["none"])
    assert all(0 < m.sum() < case.n_docs for m in masks)
    exp_bits = np.stack([filter_ref.pack(m) for m in masks])
    words = filter_ref.words(case.n_docs)
    assert L.srx_filter_from_terms_bytes(3, case.n_docs) == 3 * words * 4
    lists = [x for key in ("all", "any", "none") for x in _csr_lists(big[key])]
    bits = None
    for copies in [case.copies] + ([("post",)] if len(case.copies) == 2 else []):
        d = w.desc(base, copies)
        bits = torch.full((3, words), GARBAGE, dtype=torch.int32, device=DEV)
        run.call("srx_filter_from_terms", ctypes.byref(d), 3, *(_ptr(x) for x in lists), None, _ptr(bits), run.stream)
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), exp_bits), f"{name} srx_filter_from_terms from {copies}"
    # the filtered search through those rows, and its search-after form
    q_filter = np.array(([0, 1, 2, -1] * nq)[:nq], np.int32)
    allow = [None if f < 0 else masks[f] for f in q_filter]
    qf = _dev(q_filter)
    flt = _capi.DocFilterDesc(bits=_ptr(bits), n_filters=3, q_filter=_ptr(qf))
    exp_f = T.ranked_rows(w.full, K, base, allow=allow)
    assert any(not np.array_equal(exp_f[0][q], exp[0][q]) for q in range(nq)), "the rows restrict something"
    _assert_rows(_search(run, arena, top, "srx_search_filtered", K, extra=(ctypes.byref(flt), None, None)), exp_f, f"{name} srx_search_filtered")
    _assert_rows(_search(run, arena, top, "srx_search_filtered_packed", K, extra=(ctypes.byref(flt), None, None), packed=True), exp_f,
                 f"{name} srx_search_filtered_packed")
    exp_fa = T.ranked_rows(w.full, K, base, allow=allow, after=after)
    _assert_rows(_search(run, arena, top, "srx_search_filtered", K, extra=(ctypes.byref(flt), _ptr(ad), _ptr(as_))), exp_fa, f"{name} srx_search_filtered after")
    top.close()
    # srx_score_docs: the docs of the first page, their neighbours, ids outside the shard, padding -- from every copy
    cand = np.concatenate([exp[0], np.where(exp[0] >= 0, exp[0] + 1, -1), np.where(exp[0] > base, exp[0] - 1, -1),
                           np.tile(np.array([-1, base - 1, base + case.n_docs, T.MAX_ID + 1], np.int64), (nq, 1))], axis=1).astype(np.int32)
    m = cand.shape[1]
    cnt = np.array(([m, m, 2 * K, 3, 0] * nq)[:nq], np.int32)
    exp_s = score_ref.gather_expected(w.full, cand, cnt, base)
    assert np.count_nonzero(exp_s) > nq
    dc, dn = _dev(cand), _dev(cnt)
    for copies in [case.copies] + ([("post",)] if len(case.copies) == 2 else []):
        d = w.desc(base, copies)
        out = torch.full((nq, m), GARBAGE, dtype=torch.int32, device=DEV)
        run.call("srx_score_docs", ctypes.byref(d), *(_ptr(x) for x in w.q), nq, _ptr(dc), _ptr(dn), m, _ptr(out), run.stream)
        score_ref.assert_bits_equal(out.cpu().numpy().view(F), exp_s, f"{name} srx_score_docs from {copies}")
    # srx_build_compact over the whole canonical array: the planted blocks and the pad, and nothing else that is not 0
    if len(case.copies) == 2:
        post, post16 = w.copies["post"], w.copies["post16"]
        cw = case.words("post16")
        run.timed("fill post16 with the garbage word", lambda: post16.fill_(GARBAGE))
        run.call("srx_build_compact", 0, T.VAL_TYPE[case.val], _ptr(post), lay.n_blocks + T.BLOCK_PAD, case.tile_log2, case.unit_tiles, _ptr(post16), run.stream)
        nz = 0
        for p in lay.planted:
            e = lay.blocks_of(p["small"], "post16")
            got = post16[p["ptr"] // 4 * cw: (p["ptr"] + p["extent"]) // 4 * cw].cpu().numpy()
            assert np.array_equal(got, e.reshape(-1)), f"{name} srx_build_compact: term {p['term']}"
            nz += int(np.count_nonzero(e))
        e = lay.pad_blocks("post16")
        assert np.array_equal(post16[lay.n_blocks * cw:].cpu().numpy(), e.reshape(-1)), f"{name} srx_build_compact: the sentinel pad"
        nz += int(np.count_nonzero(e))
        got_nz = run.timed("count_nonzero post16", lambda: _count_nonzero(post16))
        assert got_nz == nz, f"{name} srx_build_compact: {got_nz} non-zero words, {nz} planted"
    run.done()


def test_build_tile_skip_past_2_31_entries(gpu):
    """srx_build_tile_skip on the shape of s-gt31: a term-major input that is empty for the filler terms and holds the planted
    postings for the planted ones; the planted rows against the lower bounds of the CSR, every other entry 0"""
    import torch
    L, arena = gpu
    case = CASES["s-gt31"]
    lay = T.build(case)
    run = Run(L, "t-build-tile-skip")
    arena.reset()
    indptr, indices, data = lay.csr
    docs = np.repeat(np.arange(case.n_docs), np.diff(indptr))
    order = np.lexsort((docs, indices))
    counts = np.zeros(lay.vocab, np.int64)
    big = np.array([p["term"] for p in lay.planted], np.int64)
    counts[big] = np.bincount(indices, minlength=len(big))
    tm_ptr = np.zeros(lay.vocab + 1, np.int64)
    np.cumsum(counts, out=tm_ptr[1:])
    assert np.all(np.diff(big) > 0), "ascending real ids: the term-major order of the small ids is the order of the real ones"
    post_doc = docs[order].astype(np.int32)
    total = lay.vocab * case.row
    assert total > 1 << 31
    out = arena.take(total * 4, torch.int32)
    run.timed("fill out_skip with the garbage word", lambda: out.fill_(GARBAGE))
    run.call("srx_build_tile_skip", 0, _ptr(_dev(tm_ptr)), _ptr(_dev(post_doc)), lay.vocab, case.n_tiles, case.tile_log2, _ptr(out), run.stream)
    edges = np.arange(case.row, dtype=np.int64) << case.tile_log2
    nz = 0
    for p in lay.planted:
        d = docs[order][tm_ptr[p["term"]]: tm_ptr[p["term"] + 1]]
        assert np.all(np.diff(d) > 0)
        e = np.searchsorted(d, edges).astype(np.int32)
        got = out[p["term"] * case.row: (p["term"] + 1) * case.row].cpu().numpy()
        assert np.array_equal(got, e), f"srx_build_tile_skip: the row of term {p['term']}"
        nz += int(np.count_nonzero(e))
    straddle = [pl for pl in lay.places if pl and "entry" in pl][0]
    t = lay.planted[straddle["small"]]["term"]
    assert t * case.row < 1 << 31 < (t + 1) * case.row and nz > 0
    got_nz = run.timed("count_nonzero out_skip", lambda: _count_nonzero(out))
    assert got_nz == nz, f"srx_build_tile_skip: {got_nz} non-zero entries, {nz} in the planted rows"
    run.done()


# ---- srx_build_blocks with an output past byte 2^32 ----------------------------------------------------------------------------------
BB_FILLERS = 16400  # filler terms of 32 764 postings each: 2^27 blocks are 2^29 postings


def test_build_blocks_past_byte_2_32(gpu):
    """Term-major arrays generated on the device: BB_FILLERS filler terms, each with a posting of value 1 on every doc below
    32 764 (a multiple of 4 in every unit: no run padding), and the planted terms of p-f32-both's first two and last groups
    at term 0, in the middle (where the output passes byte 2^32) and at the end.  Filler blocks are checked in closed form on
    the device (block b of a filler holds docs 4 b .. 4 b + 3 of its term and four ones), the planted terms against
    build_ref.layout of the planted postings."""
    import torch
    L, arena = gpu
    case = CASES["p-f32-both"]
    lay = T.build(case)
    run = Run(L, "t-build-blocks")
    arena.reset()
    cap = case.filler_cap()
    assert cap == 32764
    # the planted part: the term-major postings of three groups -- at term 0, in the middle, at the end.  In front of the middle
    # group one SHORT filler (docs below c1) so that the group starts 400 postings below byte 2^32 of the output
    groups = (0, 1, len(case.groups) - 1)
    indptr, indices, data = lay.csr
    docs_all = np.repeat(np.arange(case.n_docs), np.diff(indptr))
    smalls = [[p["small"] for p in lay.planted if p["group"] == g] for g in groups]
    padded = lambda s: int(lay.small[0][s + 1] - lay.small[0][s])  # noqa: E731  (padded postings of a planted term)
    want = (1 << 32) // 8 - 400 - sum(padded(s) for s in smalls[0])  # padded postings of the fillers in front of the middle group
    h, c1 = want // cap, want % cap
    assert 0 < h < BB_FILLERS and c1 % 4 == 0 and c1 > 0
    seg = [("planted", smalls[0]), ("fill", h, cap), ("fill", 1, c1), ("planted", smalls[1]), ("fill", BB_FILLERS - h, cap), ("planted", smalls[2])]
    vocab = BB_FILLERS + 1 + sum(len(s) for s in smalls)
    nnz = BB_FILLERS * cap + c1 + sum(int((indices == x).sum()) for s in smalls for x in s)
    post_term = arena.take(nnz * 4, torch.int32)
    post_doc = arena.take(nnz * 4, torch.int32)
    post_val = arena.take(nnz * 4, torch.float32)
    counts = np.zeros(vocab, np.int64)
    rows_c, cols_c, vals_c = [], [], []  # COO of the planted terms over the term ids of THIS index
    pos, t = 0, 0
    planted_terms, fills = {}, []
    for kind, *payload in seg:
        if kind == "fill":
            n_terms, c = payload
            n = n_terms * c
            for lo in range(0, n, 1 << 25):  # in pieces: the int64 temporaries stay small
                idx = torch.arange(lo, min(lo + (1 << 25), n), dtype=torch.int64, device=DEV)
                post_term[pos + lo: pos + lo + len(idx)] = (t + idx // c).to(torch.int32)
                post_doc[pos + lo: pos + lo + len(idx)] = (idx % c).to(torch.int32)
                del idx
            post_val[pos: pos + n] = 1.0
            counts[t: t + n_terms] = c
            fills.append((t, n_terms, c))
            pos += n
            t += n_terms
        else:
            for s in payload[0]:
                sel = indices == s
                d, v = docs_all[sel], data[sel]
                assert np.all(np.diff(d) > 0)
                post_term[pos: pos + len(d)] = t
                post_doc[pos: pos + len(d)].copy_(_dev(d.astype(np.int32)))
                post_val[pos: pos + len(d)].copy_(_dev(v))
                counts[t] = len(d)
                rows_c.append(d)
                cols_c.append(np.full(len(d), t))
                vals_c.append(v)
                planted_terms[t] = s
                pos += len(d)
                t += 1
    assert t == vocab
    assert pos == nnz
    tm_ptr = np.zeros(vocab + 1, np.int64)
    np.cumsum(counts, out=tm_ptr[1:])
    # the unpadded skip table and the run prefix: host arithmetic on [vocab, row] / [vocab, n_units] (a few MB), planted rows from the CSR
    n_units = case.n_units
    edges = np.arange(case.row, dtype=np.int64) << case.tile_log2
    skip = np.zeros((vocab, case.row), np.int32)
    run_len = np.zeros((vocab, n_units), np.int64)
    for first, n_terms, c in fills:
        skip[first: first + n_terms] = np.minimum(edges, c)
        run_len[first: first + n_terms] = np.diff(np.minimum(edges[::case.unit_tiles], c))
        assert np.all(run_len[first] % 4 == 0) and run_len[first].sum() == c
    for tt, s in planted_terms.items():
        d = docs_all[indices == s]
        skip[tt] = np.searchsorted(d, edges)
        run_len[tt] = np.diff(skip[tt][np.minimum(np.arange(n_units + 1) * case.unit_tiles, case.n_tiles)])
    runpad = np.zeros(vocab * n_units + 1, np.int64)
    np.cumsum(((run_len + 3) // 4 * 4).reshape(-1), out=runpad[1:])
    n_blocks = int(runpad[-1]) // 4
    assert n_blocks * 32 > 1 << 32 and 3 * 4 * nnz + (n_blocks + T.BLOCK_PAD) * 32 + (1 << 28) < arena.buf.numel()
    out_post = arena.take((n_blocks + T.BLOCK_PAD) * 32, torch.int32)
    run.timed("fill out_post with the garbage word", lambda: out_post.fill_(GARBAGE))
    out_skip = torch.full((vocab * case.row,), GARBAGE, dtype=torch.int32, device=DEV)
    out_tp = torch.full((vocab + 1,), GARBAGE, dtype=torch.int64, device=DEV)
    run.call("srx_build_blocks", 0, 0, _ptr(_dev(tm_ptr)), _ptr(post_term), _ptr(post_doc), _ptr(post_val), _ptr(_dev(skip.reshape(-1))), _ptr(_dev(runpad)),
             vocab, nnz, case.n_tiles, case.tile_log2, case.unit_tiles, _ptr(out_post), _ptr(out_skip), _ptr(out_tp), n_blocks, run.stream)
    exp_tp = runpad[np.arange(vocab + 1) * n_units]
    assert np.array_equal(out_tp.cpu().numpy(), exp_tp), "out_term_ptr"
    # the planted terms: build_ref.layout of the planted postings alone gives their blocks and skip rows (sentinels carry t mod 64)
    rows_c, cols_c, vals_c = np.concatenate(rows_c), np.concatenate(cols_c), np.concatenate(vals_c)
    keys = sorted(planted_terms)
    local = {tt: i for i, tt in enumerate(keys)}
    # ... over a vocabulary of 64 x planted slots so that (slot mod 64) == (real id mod 64)
    slot = {tt: 64 * local[tt] + tt % 64 for tt in keys}
    tp_r, post_r, skip_r, nb_r = build_ref.layout(rows_c, np.array([slot[int(x)] for x in cols_c]), vals_c, case.n_docs, 64 * len(keys), case.tile_log2, case.unit_tiles)
    post_r, skip_r = post_r.reshape(-1, 8), skip_r.reshape(-1, case.row)
    straddles = False
    for tt in keys:
        a, b = int(exp_tp[tt]) // 4, int(exp_tp[tt + 1]) // 4
        got = out_post[a * 8: b * 8].cpu().numpy().reshape(-1, 8)
        assert np.array_equal(got, post_r[tp_r[slot[tt]] // 4: tp_r[slot[tt] + 1] // 4]), f"srx_build_blocks: the blocks of planted term {tt}"
        assert np.array_equal(out_skip[tt * case.row: (tt + 1) * case.row].cpu().numpy(), skip_r[slot[tt]]), f"srx_build_blocks: the skip row of planted term {tt}"
        straddles |= a * 32 < 1 << 32 < b * 32
    assert straddles, "a planted term's blocks lie across byte 2^32 of the output"
    assert np.array_equal(out_post[n_blocks * 8:].cpu().numpy().reshape(-1, 8), lay.pad_blocks()), "the sentinel pad"
    # the filler terms in closed form, on the device, a span of fillers at a time
    ok_skip = True
    for first, n_terms, c in fills:
        fill_row = _dev(np.minimum(edges, c).astype(np.int32))
        ok_skip &= bool((out_skip[first * case.row: (first + n_terms) * case.row].view(n_terms, case.row) == fill_row[None, :]).all())
        a, b = int(exp_tp[first]) // 4, int(exp_tp[first + n_terms]) // 4
        assert b - a == n_terms * c // 4
        step = 1 << 24
        for lo in range(a, b, step):
            hi = min(lo + step, b)
            blk = out_post[lo * 8: hi * 8].view(hi - lo, 8)
            pos4 = (torch.arange(lo - a, hi - a, dtype=torch.int64, device=DEV) * 4) % c  # c is a multiple of 4: a block never wraps
            ok = bool((blk[:, :4] == (pos4[:, None] + torch.arange(4, device=DEV)[None, :]).to(torch.int32)).all())
            ok &= bool((blk[:, 4:] == 0x3F800000).all())
            assert ok, f"srx_build_blocks: filler blocks [{lo}, {hi})"
            del pos4
    assert ok_skip, "srx_build_blocks: a filler term's skip row"
    run.done()


# ---- the search workspace past byte 2^32 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["smallest", "scores-past"])
def test_search_workspace_past_byte_2_32(gpu, which):
    """k = 1024 on the scaled-down build of p-f32-both (a 3 MB index; the fillers' extents stay zero and unread as in the big
    cases), queries of one planted term each: the smallest batch whose workspace has a region start past byte 2^32, and the
    first batch whose score lists START there.  Every item is tier 2's (k > 112); the first n_whole queries are unsplit, the
    tail is split in two and merged by the block merge kernel.  All rows are compared on the device with the rows of the
    query's term; the worklist is read back from its place behind byte 2^32."""
    import torch
    L, arena = gpu
    case = CASES[T.WS_CASE]
    lay = T.build(case, case.shrink)
    nq, k = (T.ws_nq() if which == "smallest" else T.WS_NQ2), T.WS_K
    run = Run(L, f"w-{which}-{nq}")
    arena.reset()
    w = _plant(run, arena, lay)
    P = len(lay.planted)
    # expected rows of the P distinct queries (term, weight 1), as packed rows
    one = (np.arange(P + 1, dtype=np.int32), np.arange(P, dtype=np.int32), np.ones(P, F))
    full = T.full_scores(lay.csr, lay.idf_small, one, case.n_docs)
    base = case.doc_base_top
    ed, es, ec = T.ranked_rows(full, k, base)
    assert ec.max() == k and ec.min() < k, "full rows and padded ones"
    exp = _dev(np.concatenate([ed, es.view(np.int32), ec[:, None]], axis=1))
    big = np.array([p["term"] for p in lay.planted], np.int32)
    w.q = (_dev(np.arange(nq + 1, dtype=np.int32)), _dev(big[np.arange(nq) % P]), _dev(np.ones(nq, F)))
    w.nq = nq
    ix = Index(run, w, base)
    ix.opts(0, 0)
    p = T.ws_plan(nq)
    ws_bytes = L.srx_search_workspace_bytes(ix.h, nq, k)
    assert ws_bytes == parity.plan_workspace_bytes(p, nq, k) > 1 << 32
    ws = arena.take(ws_bytes + 4 * T.GUARD_WORDS)
    run.timed("fill workspace with the garbage word", lambda: ws.view(torch.int32).fill_(GARBAGE))
    out = arena.take(nq * (2 * k + 1) * 4, torch.int32)
    run.timed("fill rows with the garbage word", lambda: out.fill_(GARBAGE))
    run.call("srx_search_packed", ix.h, *(_ptr(x) for x in w.q), nq, k, _ptr(out), _ptr(ws), ws_bytes, run.stream)
    ix.close()
    _guard_intact(ws, ws_bytes, run.name)
    rows = out.view(nq, 2 * k + 1)
    bad = 0
    for lo in range(0, nq, 1 << 14):
        hi = min(lo + (1 << 14), nq)
        idx = torch.arange(lo, hi, device=DEV) % P
        bad += int((rows[lo:hi] != exp[idx]).any(dim=1).sum())
    assert bad == 0, f"{run.name}: {bad} of {nq} rows differ from the rows of their term"
    lay_ws = parity.search_ws(p, nq, k)
    work = ws[lay_ws["work"]: lay_ws["work"] + 4 * (1 + p["items"])].view(torch.int32)
    assert lay_ws["work"] > 1 << 32 and int(work[0]) == p["items"], f"work[0] = {int(work[0])} of {p['items']} items"
    assert bool((torch.sort(work[1:]).values == torch.arange(p["items"], device=DEV, dtype=torch.int32)).all()), "every item once on tier 2's worklist"
    assert _count_nonzero(ws[lay_ws["ovf"]: lay_ws["done"]].view(torch.int32)) == 0, "no flag bit: tier 1 serves nothing at k = 1024"
    run.done()
