"""What the doc filter of a filtered search costs: per corpus, the time of one batch

  a. unfiltered, every query through tier 2 with the score bounds off (debug bits 8 | 16): the route of a filtered search
     without the filter test -- the plain instances of the tier-2 kernel, whose code this feature leaves as it was;
  b. filtered with an all-ones row;
  c. filtered with a row of density 0.5,

each the median of ``--iters`` hipEvent-timed batches after ``--warmup``, same device tensors, same stream.

    python tools/bench_filtered.py [--corpus uniform100k|c3] [--queries N] [--iters 20] [--warmup 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparse_rx  # noqa: E402
from sparse_rx import synth  # noqa: E402

TIER2_ONLY_NO_BOUNDS = 8 | 16


def build(corpus, dev):
    if corpus == "uniform100k":  # the corpus and geometry of tests/test_search_plans.py
        c = synth.uniform_corpus_np(100_000, 5_000, 30, seed=71)
        _, idf, avgdl = synth.corpus_stats(c)
        ix = sparse_rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, device=dev,
                                            tile_log2=10, unit_tiles=4)
        return ix, 5_000, 8, 72
    n_docs, V, nnz, seed = 10_000_000, 100_000, 100, 20253  # bench.py --workload c3
    rows, cols, tfs, dls = [], [], [], []
    chunk = min(synth.CHUNK_DOCS, n_docs)
    for ci in range(n_docs // chunk):
        r, cc, tf, dl = synth.uniform_chunk_torch(ci, chunk, V, nnz, seed, dev)
        rows.append(r + ci * chunk)
        cols.append(cc)
        tfs.append(tf)
        dls.append(dl)
    rows, cols, tf, dl = torch.cat(rows), torch.cat(cols), torch.cat(tfs), torch.cat(dls)
    df = torch.bincount(cols, minlength=V).cpu().numpy()
    idf = torch.as_tensor(np.log((n_docs - df + 0.5) / (df + 0.5)).astype(np.float32), device=dev)
    ix = sparse_rx.DeviceIndex.from_coo(rows, cols, tf, idf, n_docs, doc_lengths=dl, k1=1.2, b=0.75, avgdl=float(dl.mean().item()),
                                        device=dev)
    return ix, V, 8, seed + 1


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="uniform100k", choices=["uniform100k", "c3"])
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ix, V, terms, qseed = build(a.corpus, dev)
    q = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in synth.queries_np(a.queries, V, terms, seed=qseed)]
    rng = np.random.default_rng(5)
    flt = sparse_rx.DocFilter.from_masks(np.stack([np.ones(ix.n_docs, bool), rng.random(ix.n_docs) < 0.5]), device=dev)
    rows = [torch.full((a.queries,), r, dtype=torch.int32, device=dev) for r in (0, 1)]
    out = None
    print(f"# {a.corpus}: {ix.n_docs} docs, {a.queries} queries x {terms} terms, k = {a.k}; median (min .. max) ms of {a.iters} batches after "
          f"{a.warmup} warm-up, hipEvents on the current stream; {torch.cuda.get_device_name(0)}; kernel sources "
          f"{sparse_rx._capi.kernel_sources_sha256()[:16]}", flush=True)
    ix.set_opts(debug=TIER2_ONLY_NO_BOUNDS)
    out = ix.search_device(*q, a.k)
    base = timed(lambda: ix.search_device(*q, a.k, out=out), a.iters, a.warmup)
    ix.set_opts()
    ones = timed(lambda: ix.search_device(*q, a.k, out=out, filter=flt, q_filter=rows[0]), a.iters, a.warmup)
    half = timed(lambda: ix.search_device(*q, a.k, out=out, filter=flt, q_filter=rows[1]), a.iters, a.warmup)
    plain = timed(lambda: ix.search_device(*q, a.k, out=out), a.iters, a.warmup)
    for name, t in (("unfiltered, tier 2 only, bounds off (debug 8|16)", base), ("filtered, all-ones row", ones),
                    ("filtered, density-0.5 row", half), ("plain search (both tiers, bounds on), for scale", plain)):
        print(f"{name:52s} {t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f})   {100.0 * (t[0] / base[0] - 1.0):+6.1f} % vs the first row", flush=True)
    ix.close()


if __name__ == "__main__":
    main()
