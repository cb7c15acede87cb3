#!/usr/bin/env python3
"""Measure the late-interaction search (include/late/sparse_rx_maxsim_search.h) on the GPU against the two routes a user had
before it, in the same call: ``rerank_device`` over consecutive 1 024-doc lists with a final merge (the existing route), and one
torch route (chunked half matmul, segment max by ``tok_ptr``, sum, ``topk``).  Nothing here is asserted by a test.

Store: Gaussian token rows from a seed, 40 .. 120 tokens per doc (80 on average), f16.  Timing as tools/bench_binary.py: medians
of ``--reps`` device-event timings after ``--warmup`` calls, the routes alternating inside each repetition; one JSON line per
measurement.  Before a shape is timed the search and the rerank route must return the same words; the torch route sums in another
order and in half precision, so only its overlap with the search's top k is reported.

    python tools/bench_late_search.py --docs 20000 200000 --log profiles/late_search.log
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_binary import stats, time_routes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[20_000, 200_000])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--tq", type=int, default=32)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import torch
    import sparse_rx
    if not torch.cuda.is_available():
        raise SystemExit("bench_late_search.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "a" if args.append else "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian", seed=args.seed, dim=args.dim, tq=args.tq, reps=args.reps,
         warmup=args.warmup)
    for n in args.docs:
        counts = np.random.default_rng(args.seed).integers(40, 121, n)
        n_tok = int(counts.sum())
        gen = torch.Generator(device=dev).manual_seed(args.seed)
        tok = torch.randn((n_tok, args.dim), generator=gen, device=dev, dtype=torch.float32)
        ix = sparse_rx.TokenIndex.from_token_embeddings(tok, counts, dtype="f16", device=dev)
        tok_h = tok.half()
        del tok
        torch.cuda.empty_cache()
        ptr = ix.tok_ptr.long()
        seg = torch.repeat_interleave(torch.arange(n, device=dev), torch.as_tensor(counts, device=dev))  # the doc of every token row
        queries = torch.randn((max(args.nq), args.tq, args.dim), generator=gen, device=dev, dtype=torch.float32)
        all_docs = torch.arange(n, dtype=torch.int32, device=dev)
        token_bytes = n_tok * ix.dim_pad * 2
        for nq in args.nq:
            q = queries[:nq].contiguous()
            q_h = q.half().reshape(nq * args.tq, args.dim)
            for k in args.k:
                def search():
                    return ix.search_device(q, None, k)

                def rerank_lists():  # the existing route: every 1 024-doc list reranked, the lists merged
                    docs, scores = [], []
                    for c0 in range(0, n, 1024):
                        cand = all_docs[c0: c0 + 1024].expand(nq, -1).contiguous()
                        d, s, _ = ix.rerank_device(q, None, cand, None, min(k, int(cand.shape[1])))
                        docs.append(d)
                        scores.append(s)
                    d, s = torch.cat(docs, 1), torch.cat(scores, 1)
                    s, order = torch.sort(s, dim=1, descending=True, stable=True)  # ties stay in doc order: the lists ascend
                    return torch.gather(d, 1, order)[:, :k], s[:, :k]

                def torch_route():
                    step = max(1, (1 << 28) // (nq * args.tq * 80))  # docs per chunk: a similarity block of about 2^28 halves
                    out = torch.zeros((nq, n), dtype=torch.float32, device=dev)
                    for d0 in range(0, n, step):
                        d1 = min(n, d0 + step)
                        t0, t1 = int(ptr[d0]), int(ptr[d1])
                        sim = q_h @ tok_h[t0:t1].T
                        best = torch.full((nq * args.tq, d1 - d0), float("-inf"), dtype=sim.dtype, device=dev)
                        best.scatter_reduce_(1, (seg[t0:t1] - d0).expand(nq * args.tq, -1), sim, "amax")
                        out[:, d0:d1] = best.view(nq, args.tq, d1 - d0).float().sum(1)
                    return torch.topk(out, min(k, n), dim=1)

                got, old = search(), rerank_lists()
                torch.cuda.synchronize()
                assert torch.equal(got[0], old[0]) and torch.equal(got[1].view(torch.int32), old[1].view(torch.int32)), (n, nq, k)
                tk = torch_route()
                overlap = float((got[0][:, :, None] == tk[1][:, None, :].int()).any(2).float().mean().item())
                t = time_routes(torch, {"search": search, "rerank_lists": rerank_lists, "torch": torch_route}, args.reps, args.warmup)
                for name, ms in t.items():
                    emit(what="time", n_docs=n, n_tok=n_tok, nq=nq, k=k, route=name, **stats(ms))
                med = float(np.median(t["search"]))
                emit(what="rate", n_docs=n, nq=nq, k=k, token_tb_per_s_one_pass=token_bytes / (med * 1e-3) / 1e12, top_per_s=nq / (med * 1e-3),
                     torch_topk_overlap=overlap)
                for base in ("rerank_lists", "torch"):
                    gain = float(np.median(t[base]) - med)
                    both = float(max(t[base]) - min(t[base]) + max(t["search"]) - min(t["search"]))
                    emit(what="verdict", n_docs=n, nq=nq, k=k, base=base, search_faster_by_ms=gain, combined_spread_ms=both,
                         faster_beyond_spread=bool(gain > both))
        ix.close()
        del tok_h, seg, queries
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
