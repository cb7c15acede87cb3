#!/usr/bin/env python3
"""Measure the IVF dense index (include/ivf/sparse_rx_ivf.h) on the GPU: ``IvfHalfIndex`` f16 against this project's own exhaustive
``DenseHalfIndex`` f16 search over the same rows, alternating in the same call; the bytes of rows a search actually reads against
the corpus bytes; recall@10 against the exhaustive f16 ranking; the training and build time, the list-size spread and the rate of
``srx_ivf_assign``.  Nothing here is asserted by a test, and no target is set: the yardstick is the half index of the same run.

Corpus and timing are those of tools/bench_binary.py (its Gaussian mixture; the median of ``--reps`` device-event timings after
``--warmup`` calls, the routes alternating inside every repetition, min and max printed as the spread).  IVF is called "faster"
only when the gap between the medians exceeds the two spreads together.  RECALL ON THE SYNTHETIC MIXTURE SAYS NOTHING ABOUT REAL
EMBEDDINGS.  One JSON line per measurement.

    python tools/bench_ivf.py --docs 1000000 10000000 --log profiles/ivf.log
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


def rows_read(torch, ix, probe_list):
    """Bytes of packed rows one search of this batch reads: every probed list's tiles once per group of up to 32 queries."""
    per_list = torch.bincount(probe_list[probe_list >= 0].long().flatten(), minlength=ix.nlist)
    tiles = (ix.list_tile[1:] - ix.list_tile[:-1]).long()
    return int((((per_list + 31) // 32) * tiles).sum().item()) * 32 * ix.dim_pad * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-iter", type=int, default=10)
    ap.add_argument("--train-per-list", type=int, default=64, help="training rows per list (the sample is train-per-list * nlist rows)")
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import sparse_rx
    from sparse_rx import ivf
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture of tools/bench_binary.py", centres=args.centres, sigma=args.sigma,
         seed=args.seed, dim=args.dim, reps=args.reps, warmup=args.warmup, k=args.k, recall_on_real_embeddings="not measured: the mixture says nothing about them")
    for n in args.docs:
        nlist = max(32, round(4 * n ** 0.5 / 32) * 32)
        emb, queries = mixture(torch, dev, n, max(max(args.nq), 64), args.dim, args.centres, args.sigma, args.seed)
        half = sparse_rx.DenseHalfIndex(emb, dtype="f16", device=dev)
        train_rows = min(n, args.train_per_list * nlist)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pick = torch.randperm(n, generator=torch.Generator().manual_seed(args.seed))[:train_rows].sort().values.to(dev)
        cent = ivf.train_centroids(emb[pick], nlist, "f16", args.n_iter, args.seed)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ix = sparse_rx.IvfHalfIndex(emb, nlist, dtype="f16", centroids=cent, device=dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        sizes = ix.list_sizes()
        emit(what="build", n_docs=n, nlist=nlist, train_rows=train_rows, n_iter=args.n_iter, train_s=round(t1 - t0, 3), build_s=round(t2 - t1, 3),
             list_max=int(sizes.max()), list_mean=round(float(sizes.mean()), 1), list_max_over_mean=round(float(sizes.max() / sizes.mean()), 2),
             empty_lists=int((sizes == 0).sum()), corpus_bytes=half.device_bytes(), ivf_bytes=ix.device_bytes())
        # the assign kernel alone, over 2^18 rows: 2 * rows * nlist * dim_pad operations
        a_rows = emb[: min(n, 1 << 18)]
        s = stats(time_routes(torch, {"assign": lambda: ix.assign_device(a_rows)}, args.reps, args.warmup)["assign"])
        emit(what="assign", n_docs=n, rows=int(a_rows.shape[0]), nlist=nlist, **{a: round(b, 4) for a, b in s.items()},
             mfma_Tops_per_s=round(2.0 * a_rows.shape[0] * nlist * ix.dim_pad / (s["median_ms"] * 1e-3) / 1e12, 1),
             centroid_TB_per_s=round(a_rows.shape[0] / 32 * nlist * ix.dim_pad * 2 / (s["median_ms"] * 1e-3) / 1e12, 2))
        rq = queries[:64].contiguous()
        want = half.search_device(rq, args.k)
        for nprobe in args.nprobe:
            emit(what="recall", n_docs=n, nlist=nlist, nprobe=nprobe, k=args.k, queries=64,
                 recall_vs_exhaustive_f16=round(recall(torch, ix.search_device(rq, args.k, nprobe), want, args.k), 4))
        del emb
        torch.cuda.empty_cache()
        for nq in args.nq:
            q = queries[:nq].contiguous()
            for nprobe in args.nprobe:
                t = {name: stats(ms) for name, ms in time_routes(torch, {"ivf": lambda: ix.search_device(q, args.k, nprobe),
                                                                         "f16": lambda: half.search_device(q, args.k)}, args.reps, args.warmup).items()}
                read = rows_read(torch, ix, ix.probe_device(q, nprobe)[0])
                emit(what="search", n_docs=n, nlist=nlist, nq=nq, nprobe=nprobe, k=args.k, ivf={a: round(b, 4) for a, b in t["ivf"].items()},
                     f16={a: round(b, 4) for a, b in t["f16"].items()}, against_f16=verdict(t["ivf"], t["f16"]),
                     f16_over_ivf=round(t["f16"]["median_ms"] / t["ivf"]["median_ms"], 2), rows_read_bytes=read,
                     rows_read_over_corpus=round(read / half.device_bytes(), 5), nprobe_over_nlist=round(nprobe / nlist, 5))
        del ix, half
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
