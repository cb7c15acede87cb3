#!/usr/bin/env python3
"""Measure the PQ dense index (include/pq/sparse_rx_pq.h) on the GPU: ``DensePqIndex`` at each ``--dsub`` against this project's
own ``DenseHalfIndex`` f16 search and ``DenseBinaryIndex`` Hamming search over the same rows, the three alternating in the same
call; the bandwidth by code bytes against the 8 TB/s of the part; recall@k against the exact f32 ranking for PQ alone and for
``ScreenedDenseIndex`` with a PQ and with a binary screen; the training and encode time.  Nothing here is asserted by a test, and
no target is set.

Corpus and timing are those of tools/bench_binary.py (its Gaussian mixture; the median of ``--reps`` device-event timings after
``--warmup`` calls, the routes alternating inside every repetition, min and max printed as the spread).  PQ is called "faster" or
"slower" than a route only when the gap between the medians exceeds the two spreads together.  RECALL ON THE SYNTHETIC MIXTURE
SAYS NOTHING ABOUT REAL EMBEDDINGS.  One JSON line per measurement.

    python tools/bench_pq.py --docs 1000000 10000000 --log profiles/pq.log
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

PEAK_TB_S = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--dsub", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 4, 32, 1024])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--recall-k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--recall-nq", type=int, default=64)
    ap.add_argument("--oversample", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--n-iter", type=int, default=8)
    ap.add_argument("--train-rows", type=int, default=65536)
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import sparse_rx
    from sparse_rx import pq
    if not torch.cuda.is_available():
        raise SystemExit("bench_pq.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture of tools/bench_binary.py", centres=args.centres, sigma=args.sigma,
         seed=args.seed, dim=args.dim, reps=args.reps, warmup=args.warmup, k=args.k, peak_TB_per_s=PEAK_TB_S,
         recall_on_real_embeddings="not measured: the mixture says nothing about them", lds_bank_conflicts="not measured")
    for n in args.docs:
        emb, queries = mixture(torch, dev, n, max(max(args.nq), args.recall_nq), args.dim, args.centres, args.sigma, args.seed)
        half = sparse_rx.DenseHalfIndex(emb, dtype="f16", device=dev)
        binary = sparse_rx.DenseBinaryIndex(emb, center="mean", device=dev)
        exact = sparse_rx.DenseF32Index(emb, device=dev)
        rq = queries[: args.recall_nq]
        want = {k: exact.search_device(rq, k) for k in args.recall_k}
        for k in args.recall_k:
            for o in args.oversample:
                got = sparse_rx.ScreenedDenseIndex(exact, binary, o).search_device(rq, k)
                emit(what="recall", n_docs=n, route="screen=binary", bytes_per_row=binary.device_bytes() // n, k=k, oversample=o, nq=args.recall_nq,
                     recall=round(recall(torch, got, want[k], k), 4))
        for dsub in args.dsub:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pick = torch.randperm(n, generator=torch.Generator().manual_seed(args.seed))[: min(n, args.train_rows)].sort().values.to(dev)
            cb = pq.train_codebooks(emb[pick], dsub, args.n_iter, args.seed)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ix = sparse_rx.DensePqIndex(emb, dsub=dsub, codebooks=cb, device=dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            s = stats(time_routes(torch, {"encode": lambda: ix._encode(torch, sparse_rx._capi.lib(), emb, 0)}, 3, 1)["encode"])
            emit(what="build", n_docs=n, dsub=dsub, M=ix.M, train_rows=int(pick.numel()), n_iter=args.n_iter, train_s=round(t1 - t0, 3),
                 build_s=round(t2 - t1, 3), encode_kernel_ms=round(s["median_ms"], 2), code_bytes=int(ix.codes.numel()), bytes_per_row=int(ix.codes.numel()) // n,
                 f16_bytes=half.device_bytes(), binary_bytes=binary.device_bytes(), max_row_norm=round(ix.max_row_norm(), 3))
            for k in args.recall_k:
                emit(what="recall", n_docs=n, route="pq", dsub=dsub, bytes_per_row=int(ix.codes.numel()) // n, k=k, nq=args.recall_nq,
                     recall=round(recall(torch, ix.search_device(rq, k), want[k], k), 4))
                for o in args.oversample:
                    got = sparse_rx.ScreenedDenseIndex(exact, ix, o).search_device(rq, k)
                    emit(what="recall", n_docs=n, route="screen=pq", dsub=dsub, k=k, oversample=o, nq=args.recall_nq, recall=round(recall(torch, got, want[k], k), 4))
            for nq in args.nq:
                q = queries[:nq].contiguous()
                t = time_routes(torch, {"pq": lambda: ix.search_device(q, args.k), "f16": lambda: half.search_device(q, args.k),
                                        "binary": lambda: binary.hamming_search_device(q, args.k)}, args.reps, args.warmup)
                sp, sh, sb = stats(t["pq"]), stats(t["f16"]), stats(t["binary"])
                groups = -(-nq // max(1, min(nq, 144 // ix.M)))  # the codes are read once per query group (per pass)
                emit(what="search", n_docs=n, dsub=dsub, nq=nq, k=args.k, pq={a: round(b, 4) for a, b in sp.items()}, f16={a: round(b, 4) for a, b in sh.items()},
                     binary={a: round(b, 4) for a, b in sb.items()}, query_groups=groups,
                     pq_code_TB_per_s=round(groups * ix.codes.numel() / (sp["median_ms"] * 1e-3) / 1e12, 3),
                     pq_fraction_of_peak=round(groups * ix.codes.numel() / (sp["median_ms"] * 1e-3) / 1e12 / PEAK_TB_S, 3),
                     pq_lookups_T_per_s=round(nq * n * ix.M / (sp["median_ms"] * 1e-3) / 1e12, 3),
                     pq_vs_f16=verdict(sp, sh), pq_vs_binary=verdict(sp, sb))
            del ix
        del emb, half, binary, exact
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
