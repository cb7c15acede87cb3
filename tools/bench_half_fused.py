#!/usr/bin/env python3
"""Measure ``srx_dense_search_half_fused`` (include/fused/sparse_rx_half_fused.h) on the GPU against ``srx_dense_search_half`` over
the same f16 rows, the two routes alternating in the same call.  Equal outputs are asserted before anything is timed.  Per shape:
the median of ``--reps`` device-event timings after ``--warmup`` calls, min and max as the spread; "faster" / "slower" only when
the gap between the medians exceeds the two spreads together (tools/bench_mx.py's verdict).  Read from the fused route's
workspace after a call: the survivors per query (the candidate buffers' counters) and the share of queries that overflowed.
No target is set.  One JSON line per measurement.

    python tools/bench_half_fused.py --docs 1000000 10000000 --log profiles/half_fused.log
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
    """(survivors i64[nq], overflow flags i64[nq]) of the last fused call (one pass): the header's workspace layout"""
    r = lambda b: -(-b // 256) * 256
    assert nq <= _capi.SRX_HALF_FUSED_PASS
    top = qb = nq
    lists = top * max(1, min(-(-ix.n_docs // 32) // 64, 4096 // k, 64))
    off = r(-(-top // 128) * 128 * 2048) + r(top * _capi.half_fused_sample(ix.n_docs, k) * 4) + 2 * r(lists * k * 4) + r(lists * 4) + r(top * 4)
    words = ix._ws[off: off + (top * 33 + 1) * 4].view(torch.int32).cpu().long()
    return words[: top * 32: 32][:qb], words[top * 32: top * 32 + qb]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--density", type=float, default=0.1, help="of the one filtered shape (largest nq, middle k)")
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
        raise SystemExit("bench_half_fused.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture of tools/bench_binary.py", centres=args.centres, sigma=args.sigma,
         seed=args.seed, dim=args.dim, dtype="f16", reps=args.reps, warmup=args.warmup, cap=_capi.SRX_HALF_FUSED_CAP,
         baseline="srx_dense_search_half of the same build, alternating in the same call")
    for n in args.docs:
        emb, queries = mixture(torch, dev, n, max(args.nq), args.dim, args.centres, args.sigma, args.seed)
        ix = sparse_rx.DenseHalfIndex(emb, dtype="f16", device=dev)
        del emb
        mask = torch.rand(n, generator=torch.Generator(device=dev).manual_seed(args.seed), device=dev) < args.density
        flt = sparse_rx.DocFilter.from_masks(mask.cpu().numpy())
        shapes = [(nq, k, None) for nq in args.nq for k in args.k] + [(max(args.nq), sorted(args.k)[len(args.k) // 2], flt)]
        for nq, k, f in shapes:
            q = queries[:nq].contiguous()
            want, got = ix.search_device(q, k, filter=f), ix.search_device(q, k, filter=f, fused=True)
            surv, ovf = counters(torch, _capi, ix, nq, k)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got)), (n, nq, k)
            t = time_routes(torch, {"matrix": lambda: ix.search_device(q, k, filter=f), "fused": lambda: ix.search_device(q, k, filter=f, fused=True)},
                            args.reps, args.warmup)
            m, fu = stats(t["matrix"]), stats(t["fused"])
            L = _capi.lib()
            emit(what="search", n_docs=n, nq=nq, k=k, filter_density=args.density if f is not None else None, sample=_capi.half_fused_sample(n, k),
                 matrix={a: round(b, 4) for a, b in m.items()}, fused={a: round(b, 4) for a, b in fu.items()}, fused_is=verdict(fu, m),
                 matrix_over_fused=round(m["median_ms"] / fu["median_ms"], 3), survivors_mean=round(float(surv.float().mean()), 1),
                 survivors_max=int(surv.max()), overflowed_share=round(float((ovf != 0).float().mean()), 4),
                 workspace_matrix=L.srx_dense_half_workspace_bytes(nq, n, k), workspace_fused=L.srx_dense_half_fused_workspace_bytes(nq, n, k))
        del ix
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
