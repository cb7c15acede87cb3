#!/usr/bin/env python3
"""Measure the asymmetric search of the binary dense index (include/asym/sparse_rx_binary_asym.h) on the GPU, next to the Hamming
search of the same index in the same call: the search alone (route 0 and both forced routes), the screened search at oversample 4
against the Hamming-screened one, the forced routes at small batches (the table the route-0 threshold is read from), and
recall@k of both screens against the exact f32 ranking.  Nothing here is asserted by a test.

Corpus, timing and output are those of tools/bench_binary.py (the same Gaussian mixture from the same seed; medians of ``--reps``
device-event timings after ``--warmup`` calls, the routes of a shape alternating inside each repetition; one JSON line per
measurement).  Recall on this synthetic mixture says nothing about real embeddings.

    python tools/bench_binary_asym.py --docs 1000000 10000000 --log profiles/binary_asym.log
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_binary import mixture, recall, stats, time_routes  # noqa: E402


def spread(ms):
    return max(ms) - min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 4, 32, 1024])
    ap.add_argument("--route-nq", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--oversample", type=int, default=4)
    ap.add_argument("--recall-queries", type=int, default=64)
    ap.add_argument("--recall-oversample", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import sparse_rx
    from sparse_rx import binary as bn
    if not torch.cuda.is_available():
        raise SystemExit("bench_binary_asym.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture", centres=args.centres, sigma=args.sigma, seed=args.seed,
         dim=args.dim, reps=args.reps, warmup=args.warmup, route_nq_default=sparse_rx._capi.SRX_BINARY_ASYM_ROUTE_NQ)
    for n in args.docs:
        emb, queries = mixture(torch, dev, n, max(max(args.nq), max(args.route_nq), args.recall_queries), args.dim, args.centres, args.sigma, args.seed)
        f32 = sparse_rx.DenseF32Index(emb, device=dev)
        binary = sparse_rx.DenseBinaryIndex(emb, center="mean", device=dev)
        del emb
        torch.cuda.empty_cache()
        k, m = args.k, bn.screen_pool(args.k, args.oversample, n)
        ham_sc = bn.ScreenedDenseIndex(f32, binary, args.oversample)
        asym_sc = bn.ScreenedDenseIndex(f32, binary, args.oversample, asymmetric=True)
        # ---- the search alone and as the screen, against the Hamming search in the same call
        for nq in args.nq:
            q = queries[:nq].contiguous()
            qb, qc = binary.encode_queries_device(q), binary.quantize_queries_device(q)
            routes = {"hamming": lambda: binary.hamming_search_device(None, m, q_bits=qb)}
            for r, name in ((0, "asym_route0"), (1, "asym_planes"), (2, "asym_mfma")):
                routes[name] = (lambda r=r: binary.asym_search_device(None, m, q_codes=qc, route=r))
            routes["quantize"] = lambda: binary.quantize_queries_device(q)
            routes["screened_hamming"] = lambda: ham_sc.search_device(q, k)
            routes["screened_asym"] = lambda: asym_sc.search_device(q, k)
            t = time_routes(torch, routes, args.reps, args.warmup)
            for name, ms in t.items():
                emit(what="time", n_docs=n, dim=args.dim, nq=nq, k=k, m=m, route=name, **stats(ms))
            for a, b in (("hamming", "asym_route0"), ("hamming", "asym_mfma"), ("screened_hamming", "screened_asym")):
                diff, both = float(np.median(t[b]) - np.median(t[a])), float(spread(t[a]) + spread(t[b]))
                emit(what="verdict", n_docs=n, nq=nq, base=a, route=b, slower_by_ms=diff, combined_spread_ms=both,
                     slower_beyond_spread=bool(diff > both), faster_beyond_spread=bool(-diff > both))
        # ---- the forced routes at small batches: route 0's threshold is the smallest nq from which MFMA wins beyond the spreads
        wins = {}
        for nq in args.route_nq:
            qc = binary.quantize_queries_device(queries[:nq].contiguous())
            t = time_routes(torch, {"asym_planes": lambda: binary.asym_search_device(None, m, q_codes=qc, route=1),
                                    "asym_mfma": lambda: binary.asym_search_device(None, m, q_codes=qc, route=2)}, args.reps, args.warmup)
            gain, both = float(np.median(t["asym_planes"]) - np.median(t["asym_mfma"])), float(spread(t["asym_planes"]) + spread(t["asym_mfma"]))
            wins[nq] = gain > both
            emit(what="route", n_docs=n, nq=nq, m=m, planes=stats(t["asym_planes"]), mfma=stats(t["asym_mfma"]), mfma_gain_ms=gain,
                 combined_spread_ms=both, mfma_wins=bool(wins[nq]))
        order = sorted(wins)
        from_nq = next((x for i, x in enumerate(order) if all(wins[y] for y in order[i:])), None)
        emit(what="route_threshold", n_docs=n, mfma_wins_from_nq=from_nq)
        # ---- recall against the exact f32 ranking: each search alone (its own top k) and as the screen
        q = queries[: args.recall_queries].contiguous()
        for kk in (10, 100):
            want = f32.search_device(q, kk)
            emit(what="recall_alone", n_docs=n, nq=args.recall_queries, k=kk, hamming=recall(torch, binary.hamming_search_device(q, kk), want, kk),
                 asym=recall(torch, binary.asym_search_device(q, kk), want, kk))
            for o in args.recall_oversample:
                h, a = bn.ScreenedDenseIndex(f32, binary, o), bn.ScreenedDenseIndex(f32, binary, o, asymmetric=True)
                emit(what="recall_screened", n_docs=n, nq=args.recall_queries, k=kk, oversample=o, pool=h.pool(kk),
                     hamming=recall(torch, h.search_device(q, kk), want, kk), asym=recall(torch, a.search_device(q, kk), want, kk))
        del f32, binary, ham_sc, asym_sc
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
