#!/usr/bin/env python3
"""Measure the graph dense index (include/graph/sparse_rx_graph.h) on the GPU: ``GraphHalfIndex.search`` f16 at each ``--itopk``
against ``IvfHalfIndex.search`` at each ``--nprobe`` and the exhaustive ``DenseHalfIndex.search`` over the same rows, the routes
alternating in the same call; recall@10 and recall@100 of every route against the exact f32 ranking (so the routes are compared at
equal recall, not at equal parameters); the rows a walk scores (``out_stat``); the build time per stage; the device bytes.  Nothing
here is asserted by a test, and no target is set.

Corpus and timing are those of tools/bench_binary.py (its Gaussian mixture; the median of ``--reps`` device-event timings after
``--warmup`` calls, min and max printed as the spread).  A route is called "faster" only when the gap between the medians exceeds
the two spreads together.  One workgroup serves one query: a batch of one runs on one compute unit, and that time is reported as
it is.  RECALL ON THE SYNTHETIC MIXTURE SAYS NOTHING ABOUT REAL EMBEDDINGS.  One JSON line per measurement.

    python tools/bench_graph.py --docs 1000000 10000000 --log profiles/graph.log
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_binary import mixture, recall, stats, time_routes  # noqa: E402
from bench_mx import verdict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--itopk", type=int, nargs="+", default=[32, 64, 128, 256])
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--degree", type=int, default=32)
    ap.add_argument("--builder", default="ivf")
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import time
    import torch
    import sparse_rx
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    def rounded(t):
        return {a: round(b, 4) for a, b in t.items()}

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture of tools/bench_binary.py", centres=args.centres, sigma=args.sigma,
         seed=args.seed, dim=args.dim, reps=args.reps, warmup=args.warmup, k=args.k, degree=args.degree, width=args.width, builder=args.builder,
         recall_on_real_embeddings="not measured: the mixture says nothing about them")
    for n in args.docs:
        emb, queries = mixture(torch, dev, n, max(max(args.nq), 64), args.dim, args.centres, args.sigma, args.seed)
        rq = queries[:64].contiguous()
        exact = sparse_rx.DenseF32Index(emb, device=dev)  # the f32 ranking every recall is measured against
        want = {kk: exact.search_device(rq, kk) for kk in (10, 100)}
        torch.cuda.synchronize()
        del exact
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        gx = sparse_rx.GraphHalfIndex(emb, degree=args.degree, dtype="f16", builder=args.builder, device=dev)
        torch.cuda.synchronize()
        emit(what="build", n_docs=n, degree=args.degree, builder=args.builder, total_s=round(time.perf_counter() - t0, 3),
             stage_s={a: round(b, 3) for a, b in gx.build_seconds.items()}, graph_bytes=gx.device_bytes(), rows_bytes=int(gx.corpus.numel()),
             edges_per_row=round(float((gx.graph >= 0).sum().item()) / n, 2))
        nlist = max(32, round(4 * n ** 0.5 / 32) * 32)
        ivf = sparse_rx.IvfHalfIndex(emb, nlist, dtype="f16", device=dev, train_rows=min(n, 64 * nlist))
        half = gx._rows
        emit(what="bytes", n_docs=n, graph_index=gx.device_bytes(), ivf_index=ivf.device_bytes(), exhaustive_f16=half.device_bytes())
        del emb
        torch.cuda.empty_cache()
        for L in args.itopk:
            got = {kk: gx.search_device(rq, kk, itopk=max(L, -(-kk // 32) * 32), width=args.width, with_stats=True) for kk in (10, 100)}
            st = got[10][3].float()
            emit(what="recall", route="graph", n_docs=n, itopk=L, width=args.width, recall_at_10=round(recall(torch, got[10], want[10], 10), 4),
                 recall_at_100=round(recall(torch, got[100], want[100], 100), 4), steps_mean=round(float(st[:, 0].mean()), 1),
                 rows_scored_mean=round(float(st[:, 1].mean()), 1), rows_scored_over_corpus=round(float(st[:, 1].mean()) / n, 6))
        for nprobe in args.nprobe:
            emit(what="recall", route="ivf", n_docs=n, nlist=nlist, nprobe=nprobe, recall_at_10=round(recall(torch, ivf.search_device(rq, 10, nprobe), want[10], 10), 4),
                 recall_at_100=round(recall(torch, ivf.search_device(rq, 100, nprobe), want[100], 100), 4))
        emit(what="recall", route="f16", n_docs=n, recall_at_10=round(recall(torch, half.search_device(rq, 10), want[10], 10), 4),
             recall_at_100=round(recall(torch, half.search_device(rq, 100), want[100], 100), 4))
        for nq in args.nq:
            q = queries[:nq].contiguous()
            routes = {f"graph_itopk{L}": (lambda L=L: gx.search_device(q, args.k, itopk=L, width=args.width)) for L in args.itopk}
            routes.update({f"ivf_nprobe{p}": (lambda p=p: ivf.search_device(q, args.k, p)) for p in args.nprobe})
            routes["f16"] = lambda: half.search_device(q, args.k)
            t = {name: stats(ms) for name, ms in time_routes(torch, routes, args.reps, args.warmup).items()}
            emit(what="search", n_docs=n, nq=nq, k=args.k, **{name: rounded(v) for name, v in t.items()},
                 graph_against_f16={f"itopk{L}": verdict(t[f"graph_itopk{L}"], t["f16"]) for L in args.itopk},
                 graph_against_ivf={f"itopk{L}/nprobe{p}": verdict(t[f"graph_itopk{L}"], t[f"ivf_nprobe{p}"]) for L in args.itopk for p in args.nprobe})
        del gx, ivf, half
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
