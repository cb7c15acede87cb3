"""What reranking ranked lists with a tree ensemble costs:

``srx_ltr_topk`` for 1 024 lists of m in {128, 1 024, 2 048} random docs of a 10 M-doc table, k = 10, models of 100 and 500 complete
trees of depth 6 (127 nodes each, breadth-first) over 8 features -- the score, the rank, two extras and four columns (int64, int32,
float32, int64) --, mode "sum" -- against ONE batched route in torch ops on the same GPU: gather the features, walk all trees level
by level with ``gather`` (a block of trees at a time, so that the index tensors fit), add the leaves in tree order, ``topk(dim=1)``.
The leaves are multiples of 2^-12, so the sum is exact in any order; the tool asserts that both routes give equal top-k doc ids
before anything is timed.  Each figure is the median (min .. max) of ``--iters`` hipEvent-timed repetitions after ``--warmup``, same
device tensors, same stream.

    python tools/bench_ltr.py [--iters 20] [--warmup 5] > profiles/ltr.log
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparse_rx  # noqa: E402
from sparse_rx.ltr import ForestModel, RankFn  # noqa: E402
from bench_filtered import timed  # noqa: E402

N_TABLE, NQ, DEPTH, K = 10_000_000, 1024, 6, 10
DAY = 86400
FEATURES = ["score", "rank", ("extra", 0), ("extra", 1), "date", "votes", "price", "edited"]


def line(name, t, note=""):
    print(f"{name:72s} {t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){note}", flush=True)


def complete_forest(rng, n_trees, splits):
    """``n_trees`` complete trees of depth DEPTH in breadth-first order (children of node i: 2 i + 1, 2 i + 2); ``splits``: feature ->
    (lo, hi) of its thresholds.  Returns the ForestModel and (feature [T, I], threshold [T, I], leaf [T, L]) for the torch route"""
    inner, leaves = (1 << DEPTH) - 1, 1 << DEPTH
    feat = rng.integers(0, len(splits), (n_trees, inner))
    lo, hi = np.asarray([s[0] for s in splits], np.float64), np.asarray([s[1] for s in splits], np.float64)
    thr = (lo[feat] + rng.random((n_trees, inner)) * (hi[feat] - lo[feat])).astype(np.float32)
    leaf = (rng.integers(-4096, 4097, (n_trees, leaves)) / 4096.0).astype(np.float32)
    i = np.arange(inner)
    feature = np.concatenate([feat, np.full((n_trees, leaves), -1)], axis=1).reshape(-1)
    value = np.concatenate([thr, leaf], axis=1).reshape(-1)
    left = np.tile(np.concatenate([2 * i + 1, np.zeros(leaves, np.int64)]), n_trees)
    right = np.tile(np.concatenate([2 * i + 2, np.zeros(leaves, np.int64)]), n_trees)
    mdl = ForestModel.from_arrays(feature, value, left, right, np.arange(n_trees + 1) * (inner + leaves))
    return mdl, (feat, thr, leaf)


def torch_rank(tensors, arrays, doc, score, extra, k, block=25):
    """The same step in torch ops (every position live, every doc with a value)"""
    feat, thr, leaf = arrays
    nq, m = doc.shape
    local = doc.long()
    rank = torch.arange(m, device=doc.device, dtype=torch.float32).expand(nq, m)
    X = torch.stack([score, rank, extra[:, :, 0], extra[:, :, 1], tensors["date"][local].float(), tensors["votes"][local].float(), tensors["price"][local],
                     tensors["edited"][local].float()], dim=2)
    acc = torch.zeros_like(score)
    inner = feat.shape[1]
    for t0 in range(0, feat.shape[0], block):
        f_b, th_b, lf_b = feat[t0: t0 + block], thr[t0: t0 + block], leaf[t0: t0 + block]
        tb = f_b.shape[0]
        tree = torch.arange(tb, device=doc.device).expand(nq, m, tb)
        node = torch.zeros((nq, m, tb), dtype=torch.int64, device=doc.device)
        for _ in range(DEPTH):
            x = X.gather(2, f_b[tree, node])
            node = 2 * node + 1 + (~(x <= th_b[tree, node])).long()
        out = lf_b[tree, node - inner]
        for t in range(tb):  # in tree order
            acc = acc + out[:, :, t]
    val, idx = torch.topk(score + acc, k, dim=1)
    return doc.gather(1, idx), val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    now = 1_700_000_000
    cols = {"date": now - rng.integers(0, 720 * DAY, N_TABLE).astype(np.int64), "votes": rng.integers(0, 10_000, N_TABLE).astype(np.int32),
            "price": (rng.random(N_TABLE) * 200).astype(np.float32), "edited": now - rng.integers(0, 90 * DAY, N_TABLE).astype(np.int64)}
    table = sparse_rx.FieldTable.from_columns(cols, device=dev)
    tensors = {n: torch.as_tensor(v, device=dev) for n, v in cols.items()}
    splits = [(0.1, 20.1), (0, 2048), (0, 1), (0, 1), (now - 720 * DAY, now), (0, 10_000), (0, 200), (now - 90 * DAY, now)]
    print(f"# {NQ} lists of random docs of a {N_TABLE}-doc table, four columns ({table.device_bytes() / 2 ** 20:.0f} MiB resident), 8 features, complete trees "
          f"of depth {DEPTH}, k = {K}; median (min .. max) ms of {a.iters} repetitions after {a.warmup} warm-up, hipEvents on the current stream; "
          f"{torch.cuda.get_device_name(0)}", flush=True)
    for n_trees in (100, 500):
        mdl, arrays = complete_forest(rng, n_trees, splits)
        fn = RankFn(table, mdl, FEATURES)
        arrays_t = tuple(torch.as_tensor(x, device=dev) for x in arrays)
        for m in (128, 1024, 2048):
            doc = torch.as_tensor(rng.integers(0, N_TABLE, (NQ, m)).astype(np.int32), device=dev)
            score = torch.as_tensor((rng.random((NQ, m)) * 20 + 0.1).astype(np.float32), device=dev)
            extra = torch.as_tensor(rng.random((NQ, m, 2)).astype(np.float32), device=dev)
            got, exp = fn(doc, score, None, K, extra=extra, mode="sum"), torch_rank(tensors, arrays_t, doc, score, extra, K)
            torch.cuda.synchronize()
            assert torch.equal(got[0], exp[0]), "the torch route and the kernel disagree on the top-k doc ids"
            t = timed(lambda: fn(doc, score, None, K, extra=extra, mode="sum"), a.iters, a.warmup)
            tt = timed(lambda: torch_rank(tensors, arrays_t, doc, score, extra, K), a.iters, a.warmup)
            steps = NQ * m * n_trees * DEPTH
            line(f"{n_trees} trees ({mdl.n_nodes * 16 / 1024:.0f} KiB), m = {m:4d}: srx_ltr_topk", t, f"   {steps / t[0] / 1e6:.1f} G node steps / s")
            line(f"{n_trees} trees, m = {m:4d}: torch ops on the same GPU", tt,
                 f"   kernel is {tt[0] / t[0]:.2f}x {'faster' if tt[0] >= t[0] else 'SLOWER: ratio below 1'} (spreads: kernel {t[2] - t[1]:.3f} ms, "
                 f"torch {tt[2] - tt[1]:.3f} ms; difference {tt[0] - t[0]:.3f} ms)")
    table.close()


if __name__ == "__main__":
    main()
