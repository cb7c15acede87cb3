#!/usr/bin/env python3
"""Measure the IVF-PQ dense index (include/ivfpq/sparse_rx_ivfpq.h) on the GPU: ``IvfPqIndex.search`` at each ``--nprobe`` against
this project's own ``DensePqIndex.search`` (exhaustive PQ) and ``IvfHalfIndex.search`` (the same lists over f16 rows), the three
alternating in the same call; recall@k against the exact f32 ranking alone and as the screen of ``ScreenedDenseIndex`` next to
``screen="pq"``; the device bytes of each index; the build time; and what the table copy per (query, slice) costs (the scan
timed against its own launch with no tile to read is not possible from Python, so the plan and the tiles per slice are printed
next to each time).  Nothing here is asserted by a test, and no target is set.

Corpus and timing are those of tools/bench_binary.py (its Gaussian mixture; the median of ``--reps`` device-event timings after
``--warmup`` calls, the routes alternating inside every repetition, min and max printed as the spread).  IVF-PQ is called "faster"
or "slower" than a route only when the gap between the medians exceeds the two spreads together.  RECALL ON THE SYNTHETIC MIXTURE
SAYS NOTHING ABOUT REAL EMBEDDINGS.  One JSON line per measurement.

    python tools/bench_ivfpq.py --docs 1000000 10000000 --log profiles/ivfpq.log
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_binary import mixture, recall, stats, time_routes  # noqa: E402
from bench_mx import verdict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dsub", type=int, default=8)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--recall-k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--recall-nq", type=int, default=64)
    ap.add_argument("--oversample", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--n-iter", type=int, default=8)
    ap.add_argument("--train-rows", type=int, default=262144)
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import sparse_rx
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivfpq.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture of tools/bench_binary.py", centres=args.centres, sigma=args.sigma,
         seed=args.seed, dim=args.dim, dsub=args.dsub, reps=args.reps, warmup=args.warmup, k=args.k,
         recall_on_real_embeddings="not measured: the mixture says nothing about them")
    for n in args.docs:
        nlist = int(4 * n ** 0.5)
        emb, queries = mixture(torch, dev, n, max(max(args.nq), args.recall_nq), args.dim, args.centres, args.sigma, args.seed)
        exact = sparse_rx.DenseF32Index(emb, device=dev)
        rq = queries[: args.recall_nq]
        want = {k: tuple(t.clone() for t in exact.search_device(rq, k)) for k in args.recall_k}
        built = {}
        for name, make in (("ivfpq", lambda: sparse_rx.IvfPqIndex(emb, nlist, dsub=args.dsub, n_iter=args.n_iter, train_rows=args.train_rows, seed=args.seed, device=dev)),
                           ("pq", lambda: sparse_rx.DensePqIndex(emb, dsub=args.dsub, n_iter=args.n_iter, seed=args.seed, device=dev))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            built[name] = make()
            torch.cuda.synchronize()
            emit(what="build", n_docs=n, index=name, nlist=nlist if name == "ivfpq" else None, build_s=round(time.perf_counter() - t0, 3),
                 device_bytes=built[name].device_bytes(), bytes_per_row=round(built[name].device_bytes() / n, 1))
        ix, flat = built["ivfpq"], built["pq"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ivf = sparse_rx.IvfHalfIndex(emb, nlist, dtype="f16", centroids=ix.centroids_f32, device=dev)  # the same lists over f16 rows
        torch.cuda.synchronize()
        sizes = ix.list_sizes()
        emit(what="build", n_docs=n, index="ivf_f16", nlist=nlist, build_s=round(time.perf_counter() - t0, 3), device_bytes=ivf.device_bytes(),
             bytes_per_row=round(ivf.device_bytes() / n, 1), largest_over_mean_list=round(float(sizes.max() / sizes.mean()), 2), max_list_tiles=ix.max_list_tiles,
             f32_bytes=n * args.dim * 4)
        for k in args.recall_k:
            emit(what="recall", n_docs=n, route="pq", k=k, nq=args.recall_nq, recall=round(recall(torch, flat.search_device(rq, k), want[k], k), 4))
            for o in args.oversample:
                got = sparse_rx.ScreenedDenseIndex(exact, flat, o).search_device(rq, k)
                emit(what="recall", n_docs=n, route="screen=pq", k=k, oversample=o, nq=args.recall_nq, recall=round(recall(torch, got, want[k], k), 4))
            for nprobe in args.nprobe:
                ix.default_nprobe = nprobe
                emit(what="recall", n_docs=n, route="ivfpq", nprobe=nprobe, k=k, nq=args.recall_nq,
                     recall=round(recall(torch, ix.search_device(rq, k), want[k], k), 4),
                     ivf_f16_recall=round(recall(torch, ivf.search_device(rq, k, nprobe), want[k], k), 4))
                for o in args.oversample:
                    got = sparse_rx.ScreenedDenseIndex(exact, ix, o).search_device(rq, k)
                    emit(what="recall", n_docs=n, route="screen=ivfpq", nprobe=nprobe, k=k, oversample=o, nq=args.recall_nq,
                         recall=round(recall(torch, got, want[k], k), 4))
        for nq in args.nq:
            q = queries[:nq].contiguous()
            for nprobe in args.nprobe:
                t = time_routes(torch, {"ivfpq": lambda: ix.search_device(q, args.k, nprobe), "pq": lambda: flat.search_device(q, args.k),
                                        "ivf_f16": lambda: ivf.search_device(q, args.k, nprobe)}, args.reps, args.warmup)
                si, sp, sh = stats(t["ivfpq"]), stats(t["pq"]), stats(t["ivf_f16"])
                P, S, L, ws = ix.search_plan(nq, args.k, nprobe)
                mean_tiles = nprobe * float(-(-sizes // 64).mean())  # tiles a query reads on average: what S slices share
                emit(what="search", n_docs=n, nq=nq, nprobe=nprobe, k=args.k, ivfpq={a: round(b, 4) for a, b in si.items()},
                     pq={a: round(b, 4) for a, b in sp.items()}, ivf_f16={a: round(b, 4) for a, b in sh.items()}, queries_per_pass=P, slices=S,
                     slice_capacity_tiles=L, mean_tiles_per_slice=round(mean_tiles / S, 1), table_KiB_per_slice=ix.M,
                     code_KiB_per_mean_slice=round(mean_tiles / S * 64 * (-(-ix.M // 16) * 16) / 1024, 1), workspace_MiB=round(ws / 2 ** 20, 1),
                     ivfpq_vs_pq=verdict(si, sp), ivfpq_vs_ivf_f16=verdict(si, sh))
        del ix, flat, ivf, built, emb, exact
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
