#!/usr/bin/env python3
"""Measure ``srx_dense_search_f32_batched`` (include/batched/sparse_rx_f32_batched.h) on the GPU against ``srx_dense_search_f32`` over
the same f32 rows and against the f16 half index of the same rows, the three routes alternating in the same call.  Equal outputs of
the two f32 routes are asserted before anything is timed.  Per shape: the median of ``--reps`` device-event timings after
``--warmup`` calls, min and max as the spread; "faster" / "slower" only when the gap between the medians exceeds the two spreads
together (tools/bench_mx.py's verdict).  Read from the batched route's workspace after a call: the survivors per query (the
candidate buffers' counters) and the share of queries that overflowed.  No target is set.  One JSON line per measurement.

    python tools/bench_f32_batched.py --docs 1000000 10000000 --log profiles/f32_batched.log
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_binary import mixture, stats, time_routes  # noqa: E402
from bench_mx import verdict  # noqa: E402


def counters(torch, _capi, ix, nq, k):
    """(survivors i64[nq], overflow flags i64[nq]) of the last batched call (one pass): the header's workspace layout"""
    r = lambda b: -(-b // 256) * 256
    assert nq <= _capi.SRX_F32_BATCHED_PASS
    lists = nq * max(1, min(-(-ix.n_docs // 256) // 16, 4096 // k, 64))
    off = 256 + r(nq * 8) + r(nq * 4) + r(nq * _capi.f32_batched_sample(ix.n_docs, k) * 4) + 2 * r(lists * k * 4) + r(lists * 4)
    words = ix._ws[off: off + (nq * 33 + 1) * 4].view(torch.int32).cpu().long()
    return words[: nq * 32: 32], words[nq * 32: nq * 32 + nq]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 4, 32, 1024])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import sparse_rx
    from sparse_rx import _capi
    if not torch.cuda.is_available():
        raise SystemExit("bench_f32_batched.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "a") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture of tools/bench_binary.py", centres=args.centres, sigma=args.sigma,
         seed=args.seed, dim=args.dim, reps=args.reps, warmup=args.warmup, cap=_capi.SRX_F32_BATCHED_CAP, target=_capi.SRX_F32_BATCHED_TARGET,
         baseline="srx_dense_search_f32 and the f16 srx_dense_search_half of the same build, alternating in the same call")
    for n in args.docs:
        emb, queries = mixture(torch, dev, n, max(args.nq), args.dim, args.centres, args.sigma, args.seed)
        ix = sparse_rx.DenseF32Index(emb, device=dev)
        half = sparse_rx.DenseHalfIndex(emb, dtype="f16", device=dev)
        del emb
        for nq in args.nq:
            for k in args.k:
                q = queries[:nq].contiguous()
                want, got = ix.search_device(q, k), ix.search_device(q, k, batched=True)
                surv, ovf = counters(torch, _capi, ix, nq, k)
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got)), (n, nq, k)
                t = time_routes(torch, {"matvec": lambda: ix.search_device(q, k), "batched": lambda: ix.search_device(q, k, batched=True),
                                        "half": lambda: half.search_device(q, k)}, args.reps, args.warmup)
                m, b, h = stats(t["matvec"]), stats(t["batched"]), stats(t["half"])
                emit(what="search", n_docs=n, nq=nq, k=k, sample=_capi.f32_batched_sample(n, k), matvec={a: round(v, 4) for a, v in m.items()},
                     batched={a: round(v, 4) for a, v in b.items()}, half_f16={a: round(v, 4) for a, v in h.items()}, batched_is=verdict(b, m),
                     matvec_over_batched=round(m["median_ms"] / b["median_ms"], 3), survivors_mean=round(float(surv.float().mean()), 1),
                     survivors_max=int(surv.max()), overflowed_share=round(float((ovf != 0).float().mean()), 4),
                     workspace_batched=_capi.lib().srx_dense_f32_batched_workspace_bytes(nq, n, k))
        del ix, half
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
