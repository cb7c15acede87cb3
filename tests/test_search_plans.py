"""Oracle parity for every plan the search planner picks, and for searches in flight on several streams at once.

A batch is not searched by one code path: make_plan (csrc/sparse_rx.hip) cuts it into whole queries and doc-range splits
from nq, k, the unit count and target_blocks; the split queries are merged inside the tier-1 kernel (the last split to
arrive) or by one of two merge kernels; the tier-2 grid is sized by a hint the previous search left.  Every case here is
labelled with its plan (tests/parity.py: plan, a restatement of make_plan pinned to the library through
srx_search_workspace_bytes) and asserts that it lands in the bucket it was written for, then compares the rows with the
oracle bit for bit.  Run as a script (``python tests/test_search_plans.py graph-lanes``) the file is the child process of
the HIP-graph lane test."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402  (checker only)
from parity import plan, plan_label, plan_workspace_bytes, t2_grid  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_LOG2, UNIT_TILES = 10, 4  # 1 024-doc tiles, 4-tile units: a 100 k-doc corpus has 25 units, room for every split count
CORPORA = {  # name: (n_docs, kind, vocab, nnz / draws per doc, seed, build options)
    "uniform": (100_000, "uniform", 5_000, 30, 71, {}),
    "zipf": (100_000, "zipf", 20_000, 40, 72, {}),
    "small": (20_000, "uniform", 3_000, 30, 73, {}),  # 5 units: the C3 plan in miniature
    "compact": (100_000, "uniform", 5_000, 30, 71, {"keep_canonical": False, "doc_base": 5_000}),  # tier 2 reads the compact copy
    "dot16": (60_000, "splade", 3_000, 60, 74, {"mode": "dot", "val_dtype": "f16", "doc_base": 777}),
}


def _n_tiles(name):
    return (CORPORA[name][0] + (1 << TILE_LOG2) - 1) >> TILE_LOG2


def _doc_base(name):
    return CORPORA[name][5].get("doc_base", 0)


class _Env:
    """The corpora and their indexes, built once for the module."""

    def __init__(self):
        self.corpora, self.indexes = {}, {}

    def corpus(self, name):
        if name not in self.corpora:
            from sparse_rx import synth
            n, kind, V, per_doc, seed, _ = CORPORA[name]
            if kind == "uniform":
                c = synth.uniform_corpus_np(n, V, per_doc, seed=seed)
            elif kind == "zipf":
                c = synth.zipf_corpus_np(n, V, per_doc, seed=seed, s=1.0)
            else:
                c = synth.splade_corpus_np(n, V, per_doc, seed=seed)
            if kind == "splade":
                idf, avgdl, mode = np.ones(V, np.float32), 1.0, oracle.MODE_TFIDF_F32
            else:
                _, idf, avgdl = synth.corpus_stats(c)
                mode = oracle.MODE_BM25_F32
            self.corpora[name] = (c, idf, avgdl, mode)
        return self.corpora[name]

    def index(self, name):
        if name not in self.indexes:
            import sparse_rx
            c, idf, avgdl, _ = self.corpus(name)
            ix = sparse_rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl,
                                                tile_log2=TILE_LOG2, unit_tiles=UNIT_TILES, **CORPORA[name][5])
            assert ix.n_tiles == _n_tiles(name) and ix.unit_tiles == UNIT_TILES
            self.indexes[name] = ix
        return self.indexes[name]

    def oracle(self, name, q, k):
        c, idf, avgdl, mode = self.corpus(name)
        ed, es, ec = oracle.search_batch(c.indptr, c.indices, c.data, c.doc_lengths, idf, q[0], q[1], q[2], k, 1.2, 0.75, avgdl, mode=mode)
        base = _doc_base(name)
        return np.where(ed >= 0, ed + base, ed).astype(np.int32), es, ec

    def queries(self, name, nq, kind, seed):
        from sparse_rx import synth
        V = CORPORA[name][2]
        if kind == "u8":
            return synth.queries_np(nq, V, 8, seed=seed)
        if kind == "zipf8":  # hot terms: dense units, flagged to tier 2
            return synth.queries_np(nq, V, 8, seed=seed, dist="zipf", s=1.0)
        if kind == "long100":  # > 64 terms: tier 1 cannot take the query
            return synth.queries_np(nq, V, 100, seed=seed)
        if kind == "learned20":
            return synth.queries_np(nq, V, 20, seed=seed, dist="zipf", s=0.7, weights="learned")
        raise ValueError(kind)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import sparse_rx
    sparse_rx._capi.lib()
    e = _Env()
    yield e
    for ix in e.indexes.values():
        ix.close()


def _assert_exact(got, exp, label=""):
    from test_gpu_parity import _assert_exact as check
    check(got, exp, label)


def _pinned_plan(ix, name, nq, k, target, expect):
    """The restated plan of a case, checked against the library's planner (workspace size) and against its bucket."""
    p = plan(_n_tiles(name), UNIT_TILES, nq, k, target)
    assert plan_workspace_bytes(p, nq, k) == ix.workspace_bytes(nq, k), f"restated planner drifted from make_plan ({name} nq={nq} k={k})"
    for key, want in expect.items():
        assert p[key] == want, f"{name} nq={nq} k={k} target={target}: plan {key} = {p[key]}, the case was written for {want}"
    return p


def _search_layouts(ix, q, k):
    """The same batch through search_device (rows of stride k) and search_packed_device (rows of stride 2k + 1)."""
    import torch
    dq = [torch.as_tensor(np.ascontiguousarray(x), device=ix.device) for x in q]
    d, s, c = ix.search_device(*dq, k)
    packed = ix.search_packed_device(*dq, k)
    torch.cuda.synchronize()
    rows = packed.cpu().numpy()
    return ((d.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()),
            (rows[:, :k].copy(), rows[:, k:2 * k].copy().view(np.float32), rows[:, 2 * k].copy()))


# (corpus, nq, k, target_blocks, queries, the bucket the case is written for)
_MIXED = dict(n_whole=32)
CASES = [
    # mixed plans: 32 whole queries and a tail of 2 / 3 / 4 splits per query
    ("uniform", 40, 100, 16, "u8", dict(_MIXED, n_splits=2, tail=8, merge_kernel="wave", in_kernel_merge=True)),
    ("uniform", 37, 100, 16, "u8", dict(_MIXED, n_splits=3, tail=5, merge_kernel="wave", in_kernel_merge=True)),
    ("uniform", 36, 100, 16, "u8", dict(_MIXED, n_splits=4, tail=4, merge_kernel="wave", in_kernel_merge=True)),
    ("uniform", 35, 10, 16, "u8", dict(_MIXED, n_splits=4, tail=3)),
    # every query split / none split (nq a multiple of the target: n_whole falls back to 0, ns = 1)
    ("uniform", 16, 100, 64, "u8", dict(n_whole=0, n_splits=4, merge_kernel="wave")),
    ("uniform", 16, 10, 0, "u8", dict(n_whole=0, n_splits=25, merge_kernel="wave")),
    ("uniform", 16, 100, 0, "u8", dict(n_whole=0, n_splits=20, merge_kernel="block")),
    ("uniform", 32, 100, 16, "u8", dict(n_whole=0, n_splits=1)),
    # the C3 plan in miniature: default target, 3 100 queries = one whole round of 3 072 + a tail of 28 x 4 splits
    ("small", 3100, 100, 0, "u8", dict(n_whole=3072, tail=28, n_splits=4, merge_kernel="wave", in_kernel_merge=True)),
    # both merge kernels on split tails, on both sides of lists_per_q * k = 1024
    ("uniform", 16, 64, 128, "u8", dict(n_splits=8, merge_kernel="wave")),
    ("uniform", 16, 64, 144, "u8", dict(n_splits=9, merge_kernel="block")),
    ("uniform", 16, 65, 112, "u8", dict(n_splits=7, merge_kernel="wave")),
    ("uniform", 16, 65, 128, "u8", dict(n_splits=8, merge_kernel="block")),
    ("uniform", 16, 128, 64, "u8", dict(n_splits=4, merge_kernel="wave")),
    ("uniform", 16, 128, 80, "u8", dict(n_splits=5, merge_kernel="block")),
    # tier-2 work inside the tail splits: hot-term units, > 64-term queries, k > 112
    ("zipf", 37, 100, 16, "zipf8", dict(_MIXED, n_splits=3)),
    ("zipf", 36, 50, 16, "zipf8", dict(_MIXED, n_splits=4)),
    ("uniform", 37, 100, 16, "long100", dict(_MIXED, n_splits=3)),
    ("zipf", 37, 200, 16, "zipf8", dict(_MIXED, n_splits=3, t2_everything=True, merge_kernel="block")),
    # value types / layouts: f16 dot mode and the compact copy only, both with a doc_base
    ("dot16", 37, 100, 16, "learned20", dict(_MIXED, n_splits=3)),
    ("dot16", 16, 1000, 64, "learned20", dict(n_splits=2, merge_kernel="block", t2_everything=True)),
    ("compact", 37, 100, 16, "u8", dict(_MIXED, n_splits=3)),
    ("compact", 36, 113, 16, "u8", dict(_MIXED, n_splits=4, t2_everything=True)),
    ("compact", 36, 112, 16, "zipf8", dict(_MIXED, n_splits=4)),
]
# the k boundaries on one mixed plan (32 whole + 4 x the splits the cap 4096 // 2k allows)
for _k in (1, 64, 65, 111, 112, 113, 127, 128, 129, 512, 513, 1024):
    CASES.append(("uniform", 36, _k, 16, "u8", dict(_MIXED, n_splits=min(4, 4096 // (2 * _k)),
                                                    merge_kernel="wave" if _k <= 128 else "block", t2_everything=_k > 112)))


def _case_id(case):
    name, nq, k, target, qk, _ = case
    return f"{name}-nq{nq}-T{target}-{plan_label(plan(_n_tiles(name), UNIT_TILES, nq, k, target), k)}-{qk}"


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_plan_vs_oracle(env, case):
    name, nq, k, target, qk, expect = case
    label = _case_id(case)
    ix = env.index(name)
    ix.set_opts(target_blocks=target)
    p = _pinned_plan(ix, name, nq, k, target, expect)
    q = env.queries(name, nq, qk, seed=1000 + nq + 7 * k + target)
    exp = env.oracle(name, q, k)
    rows, packed = _search_layouts(ix, q, k)
    _assert_exact(rows, exp, f"{label} search_device")
    _assert_exact(packed, exp, f"{label} search_packed_device")
    if p["merge_kernel"] == "wave":
        # the same batch with the block merge kernel in the wave kernel's place (debug bit 256): the block kernel on a split
        # tail that starts at query n_whole, with the index's doc_base, which it otherwise only sees for k > 128
        ix.set_opts(target_blocks=target, debug=256)
        try:
            rows, packed = _search_layouts(ix, q, k)
        finally:
            ix.set_opts(target_blocks=target, debug=0)
        _assert_exact(rows, exp, f"{label} search_device, block merge kernel")
        _assert_exact(packed, exp, f"{label} search_packed_device, block merge kernel")


def test_search_after_pages_on_a_mixed_plan(env):
    """k = 1500 > max_k: page 1 (k = 1024) and page 2 (srx_search_after, k = 476) both on mixed plans of 32 whole queries."""
    ix = env.index("uniform")
    ix.set_opts(target_blocks=16)
    _pinned_plan(ix, "uniform", 37, 1024, 16, dict(_MIXED, n_splits=2, merge_kernel="block"))
    _pinned_plan(ix, "uniform", 37, 1500 - 1024, 16, dict(_MIXED, n_splits=3, merge_kernel="block"))
    q = env.queries("uniform", 37, "u8", seed=3)
    exp = env.oracle("uniform", q, 1500)
    assert np.all(exp[2] == 1500)  # deep enough that the second page is full too
    _assert_exact(ix.search(*q, 1500), exp, "mixed32+5x2 k=1500 paged")


def test_small_tier2_grid_drains_a_long_worklist(env):
    """A batch that leaves the tier-2 worklist empty, then a tier-2-heavy batch on the same index: search_impl reads the
    hint 0 and launches tier 2 with 128 workgroups, which must drain thousands of work items."""
    from sparse_rx import synth
    ix = env.index("zipf")
    ix.set_opts(target_blocks=0)
    c = env.corpus("zipf")[0]
    df = synth.corpus_stats(c)[0]
    rare = np.flatnonzero((df >= 1) & (df <= 20)).astype(np.int32)
    assert len(rare) >= 64
    # single rare terms, k <= 112: a few postings per unit, nothing a tier-1 wave hands on -- the worklist stays empty
    q0 = (np.arange(65, dtype=np.int32), rare[:64].copy(), np.ones(64, np.float32))
    _pinned_plan(ix, "zipf", 64, 10, 0, dict(n_whole=0, t2_everything=False))
    _assert_exact(ix.search(*q0, 10), env.oracle("zipf", q0, 10), "rare single terms")  # synchronises: the hint is 0 now
    q1 = env.queries("zipf", 200, "zipf8", seed=11)
    p = _pinned_plan(ix, "zipf", 200, 100, 0, dict(n_splits=15, t2_everything=False))
    assert p["items"] == 3000 and p["t2_full"] > 128 and t2_grid(p, 0) == 128
    _assert_exact(ix.search(*q1, 100), env.oracle("zipf", q1, 100), "hot terms after an empty worklist (128-block tier-2 grid)")


def test_split_queries_on_four_streams(env):
    """Four streams, each with a workspace of its own, six rounds of split-heavy batches (k <= 112: the in-kernel merge)
    launched back to back without a synchronisation; one batch per round is a mixed plan.  The split that arrives last
    reads the other splits' lists across XCDs (wave_kernel.hip, the hand-off after s_waitcnt): a lost store shows up here."""
    import torch
    ix = env.index("uniform")
    target = 32
    ix.set_opts(target_blocks=target)
    rng = np.random.default_rng(77)
    streams = [torch.cuda.Stream() for _ in range(4)]
    jobs = []
    for r in range(6):
        for si in range(4):
            nq = int(rng.choice([33, 37, 40, 45, 50, 57, 63])) if si == 0 else int(rng.integers(8, 17))
            k = int(rng.choice([10, 50, 100, 112]))
            p = _pinned_plan(ix, "uniform", nq, k, target, dict(in_kernel_merge=True))
            assert (p["n_whole"] > 0) == (si == 0)
            q = env.queries("uniform", nq, "u8", seed=500 + 4 * r + si)
            dq = [torch.as_tensor(x, device=ix.device) for x in q]
            out = torch.full((nq, 2 * k + 1), -7, dtype=torch.int32, device=ix.device)
            jobs.append((r, si, q, k, dq, out))
    ws = [torch.empty(max(ix.workspace_bytes(j[4][0].numel() - 1, j[3]) for j in jobs if j[1] == si), dtype=torch.uint8,
                      device=ix.device) for si in range(4)]
    torch.cuda.synchronize()
    for r, si, q, k, dq, out in jobs:
        ix.search_packed_device(*dq, k, out=out, stream=streams[si], workspace=ws[si])
    torch.cuda.synchronize()
    for r, si, q, k, dq, out in jobs:
        rows = out.cpu().numpy()
        got = (rows[:, :k], rows[:, k:2 * k].copy().view(np.float32), rows[:, 2 * k])
        _assert_exact(got, env.oracle("uniform", q, k), f"round {r} stream {si} nq={len(q[0]) - 1} k={k}")


@pytest.mark.parametrize("zero_copy", [True, False], ids=["zero_copy", "copies"])
def test_multi_stream_pipeline(env, zero_copy):
    """HostBatchPipeline(multi_stream=True, depth=4): four batches in flight on four streams, a large batch followed by
    smaller ones whose plans need a larger workspace (a slot's workspace is regrown: index.py, submit)."""
    import sparse_rx
    ix = env.index("uniform")
    ix.set_opts(target_blocks=0)
    k, max_q = 100, 200
    sizes = [200, 160, 8, 37, 150, 1, 199, 64, 170, 12]
    base_ws = ix.workspace_bytes(max_q, k)
    grows = [n for n in sizes if ix.workspace_bytes(n, k) > base_ws]
    assert grows, "no batch of the list makes a slot regrow its workspace"
    for n in sizes:
        _pinned_plan(ix, "uniform", n, k, 0, {})
    batches = [env.queries("uniform", n, "u8", seed=900 + i) for i, n in enumerate(sizes)]
    pipe = sparse_rx.HostBatchPipeline(ix, max_q, max_q * 8, k, depth=4, zero_copy_queries=zero_copy,
                                       zero_copy_results=zero_copy, multi_stream=True)
    tickets, got = [], []
    for b in batches:
        tickets.append(pipe.submit(*b))
        if len(tickets) == 4:
            got.append(tuple(x.copy() for x in pipe.result(tickets.pop(0))))
    while tickets:
        got.append(tuple(x.copy() for x in pipe.result(tickets.pop(0))))
    assert max(s["ws"].numel() for s in pipe.slots) > base_ws  # the regrowth path ran
    pipe.close()
    for n, b, g in zip(sizes, batches, got):
        _assert_exact(g, env.oracle("uniform", b, k), f"multi-stream pipeline zero_copy={zero_copy} nq={n}")


# ---- HIP-graph lanes of ShardedSearcher (a child process: a tear-down hang becomes a failed test with its output) ---------
GRAPH_CHILD_TIMEOUT = 180


def test_graph_lanes_follow_the_callers_stream():
    """ShardedSearcher's graph lanes (the default of bench.py --gpus N) replay on streams of their own.  A caller that
    refills its fixed query buffers on its own stream must get the rows of the new queries: the replay has to wait for the
    caller's stream.  Also: fresh tensors on every call do not grow the lane cache without bound."""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "graph-lanes"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=GRAPH_CHILD_TIMEOUT)
    out = p.stdout[-6000:] + "\n--- stderr ---\n" + p.stderr[-6000:]
    assert p.returncode == 0, out
    assert "graph lanes OK" in p.stdout, out


def _graph_lanes_child() -> int:
    import torch
    import torch.distributed as dist
    import sparse_rx
    from sparse_rx import synth
    from test_gpu_parity import _assert_exact as check

    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    dev = torch.device("cuda", 0)
    base, k, nq, nt = 1000, 50, 37, 8
    c = synth.uniform_corpus_np(100_000, 5_000, 30, seed=81)
    _, idf, avgdl = synth.corpus_stats(c)
    ix = sparse_rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, device=dev,
                                        tile_log2=TILE_LOG2, unit_tiles=UNIT_TILES, doc_base=base)
    ix.set_opts(target_blocks=16)  # 32 whole queries + 5 x 3 splits: the in-kernel merge inside the captured step
    rng = np.random.default_rng(82)
    batches = []
    for _ in range(6):  # the same q_ptr (nt terms per query), other terms and weights: one set of fixed buffers fits all
        t = np.sort(np.stack([rng.choice(c.vocab, nt, replace=False) for _ in range(nq)]), axis=1).astype(np.int32).reshape(-1)
        w = np.where(rng.random(nq * nt) < 0.1, 2.0, 1.0).astype(np.float32)
        batches.append((np.arange(nq + 1, dtype=np.int32) * nt, t, w))
    exps = []
    for b in batches:
        ed, es, ec = oracle.search_batch(c.indptr, c.indices, c.data, c.doc_lengths, idf, b[0], b[1], b[2], k, 1.2, 0.75, avgdl)
        exps.append((np.where(ed >= 0, ed + base, -1).astype(np.int32), es, ec))
    searcher = sparse_rx.ShardedSearcher.for_device_index(ix)
    searcher.force_exchange, searcher.graph = True, True
    qp = torch.as_tensor(batches[0][0], device=dev)
    qt = torch.empty(nq * nt, dtype=torch.int32, device=dev)
    qw = torch.empty(nq * nt, dtype=torch.float32, device=dev)
    src = [(torch.as_tensor(b[1], device=dev), torch.as_tensor(b[2], device=dev)) for b in batches]
    torch.cuda.synchronize()
    failures = []

    def fail(msg):  # printed when found: the parent shows the child's output
        print("GRAPH LANE FAILURE:", msg, flush=True)
        failures.append(msg)

    outs = []
    for bt, bw in src:
        torch.cuda._sleep(50_000_000)  # the caller's stream is busy ...
        qt.copy_(bt)  # ... when it refills the fixed buffers, behind the sleep
        qw.copy_(bw)
        o = searcher.search(qp, qt, qw, k)
        searcher.wait()
        outs.append(tuple(x.clone() for x in o))
    torch.cuda.synchronize()
    if not searcher.graph or len(searcher._lanes) != 1:
        fail(f"the graph lanes did not run (graph={searcher.graph}, lane sets={len(searcher._lanes or {})})")
    for i, (o, e) in enumerate(zip(outs, exps)):
        try:
            check(tuple(x.contiguous().cpu().numpy() for x in o), e, f"fixed buffers, batch {i}")
        except AssertionError as err:
            fail(str(err).splitlines()[0])
    bound = getattr(searcher, "LANE_KEYS", 4)
    for i in range(bound + 3):  # fresh tensors every call: a new lane set each time, the oldest released
        b = batches[i % len(batches)]
        fresh = [torch.as_tensor(x, device=dev) for x in b]
        o = searcher.search(*fresh, k)
        searcher.wait()
        got = tuple(x.contiguous().cpu().numpy() for x in o)
        try:
            check(got, exps[i % len(batches)], f"fresh tensors, call {i}")
        except AssertionError as err:
            fail(str(err).splitlines()[0])
        if len(searcher._lanes) > bound:
            fail(f"lane cache holds {len(searcher._lanes)} tensor sets after call {i} (bound {bound})")
    searcher.close()
    ix.close()
    dist.destroy_process_group()
    if failures:
        return 1
    print("graph lanes OK", flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1:] == ["graph-lanes"]:
        sys.exit(_graph_lanes_child())
    sys.exit(f"usage: {sys.argv[0]} graph-lanes")
