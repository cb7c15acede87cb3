#!/usr/bin/env python3
"""Measure the MX dense index (include/mx/sparse_rx_mx.h) on the GPU: ``DenseMxIndex`` MXFP8 and MXFP4 against this project's own
``DenseHalfIndex`` f16 search on the same rows, in the same call, and against a torch f16 ``matmul`` + ``topk`` route; and
recall@10 / @100 of both types against the exact f32 ranking.  Nothing here is asserted by a test, and no target is set: the
yardstick is the half index of the same run.

Corpus and timing are those of tools/bench_binary.py (its Gaussian mixture; the median of ``--reps`` device-event timings after
``--warmup`` calls, the routes alternating inside every repetition, min and max printed as the spread).  A route is called
"faster" than f16 only when the gap between the medians exceeds the two spreads together; otherwise the line says "no
difference measured" or "slower".  One JSON line per measurement.

    python tools/bench_mx.py --docs 1000000 10000000 --log profiles/mx.log
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_binary import PEAK_BYTES_PER_S, mixture, recall, stats, time_routes  # noqa: E402


def verdict(mx, half):
    gap = half["median_ms"] - mx["median_ms"]
    spread = (mx["max_ms"] - mx["min_ms"]) + (half["max_ms"] - half["min_ms"])
    return "faster" if gap > spread else "slower" if -gap > spread else "no difference measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 4, 32, 1024])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-max-cells", type=int, default=1 << 31, help="largest nq * n_docs the torch route is run at")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import sparse_rx
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture of tools/bench_binary.py", centres=args.centres,
         sigma=args.sigma, seed=args.seed, dim=args.dim, reps=args.reps, warmup=args.warmup, quality_on_real_embeddings="not measured")
    for n in args.docs:
        emb, queries = mixture(torch, dev, n, max(args.nq), args.dim, args.centres, args.sigma, args.seed)
        ix = {"f16": sparse_rx.DenseHalfIndex(emb, dtype="f16", device=dev), "mxfp8": sparse_rx.DenseMxIndex(emb, dtype="mxfp8", device=dev),
              "mxfp4": sparse_rx.DenseMxIndex(emb, dtype="mxfp4", device=dev)}
        # recall against the exact f32 ranking, before the f32 rows are dropped
        f32 = sparse_rx.DenseF32Index(emb, device=dev)
        rq = queries[: min(64, queries.shape[0])].contiguous()
        for k in (10, 100):
            want = f32.search_device(rq, k)
            emit(what="recall", n_docs=n, k=k, queries=int(rq.shape[0]), **{name: round(recall(torch, x.search_device(rq, k), want, k), 4) for name, x in ix.items()})
        del f32
        half_docs = emb.to(torch.float16)
        del emb
        torch.cuda.empty_cache()
        emit(what="index", n_docs=n, **{f"{name}_bytes": x.device_bytes() for name, x in ix.items()})
        for nq in args.nq:
            q = queries[:nq].contiguous()
            qh = q.to(torch.float16)
            for k in args.k:
                routes = {name: (lambda x=x: x.search_device(q, k)) for name, x in ix.items()}
                if nq * n <= args.torch_max_cells:
                    routes["torch_f16_matmul_topk"] = lambda: torch.topk(qh @ half_docs.T, k, dim=1)
                t = {name: stats(ms) for name, ms in time_routes(torch, routes, args.reps, args.warmup).items()}
                for name, s in t.items():
                    row = dict(what="search", route=name, n_docs=n, nq=nq, k=k, **{a: round(b, 4) for a, b in s.items()})
                    if name in ix:
                        if nq <= 32:  # memory-bound: the corpus is streamed once
                            row["corpus_TB_per_s"] = round(ix[name].device_bytes() / (s["median_ms"] * 1e-3) / 1e12, 3)
                            row["of_roofline"] = round(ix[name].device_bytes() / (s["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 3)
                        else:  # compute-bound: 2 * nq * n * dim_pad operations
                            row["mfma_Tops_per_s"] = round(2.0 * nq * n * ix[name].dim_pad / (s["median_ms"] * 1e-3) / 1e12, 1)
                        if name != "f16":
                            row["against_f16"] = verdict(s, t["f16"])
                            row["f16_over_this"] = round(t["f16"]["median_ms"] / s["median_ms"], 3)
                    emit(**row)
        del ix, half_docs
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
