#!/usr/bin/env python3
"""Measure the binary dense index (include/binary/sparse_rx_binary.h) on the GPU: the Hamming search alone and the screened
search (``ScreenedDenseIndex``) against this project's own exact f32 and f16 searches at the same shape on the same card, and
against one batched torch route (+-1 f16 matmul + ``topk``), whose top-m distance multisets must equal the Hamming search's.
Also recall@k of the screened search against the exact f32 search.  Nothing here is asserted by a test.

Corpus: a Gaussian mixture, generated on the device from ``torch.Generator(device).manual_seed(seed)``: ``--centres`` centres
~ N(0, I), every row = a uniformly drawn centre + N(0, sigma^2 I); the queries are drawn the same way.  Rows are generated in
chunks of 2^20, centres first, then per chunk the assignment and the noise, then the queries.

Every time is the median of ``--reps`` device-event timings of one call (after ``--warmup`` calls), the routes of a shape
alternating inside each repetition; min and max are printed as the spread.  One JSON line per measurement.

    python tools/bench_binary.py --docs 1000000 10000000 --log profiles/binary.log
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8.0e12        # HBM roofline the byte figures are set against
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9  # the VALU issue bound: one wave64 instruction per 2 cycles per SIMD


def mixture(torch, dev, n, nq, dim, centres, sigma, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    c = torch.randn((centres, dim), generator=g, device=dev)
    emb = torch.empty((n, dim), dtype=torch.float32, device=dev)
    for lo in range(0, n, 1 << 20):
        m = min(1 << 20, n - lo)
        a = torch.randint(0, centres, (m,), generator=g, device=dev)
        emb[lo: lo + m] = c[a] + sigma * torch.randn((m, dim), generator=g, device=dev)
    a = torch.randint(0, centres, (nq,), generator=g, device=dev)
    return emb, c[a] + sigma * torch.randn((nq, dim), generator=g, device=dev)


def time_routes(torch, routes, reps, warmup):
    """{name: fn} -> {name: [ms per call]}; the routes alternate inside every repetition"""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b))
    return out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def recall(torch, got, want, k):
    hit = (got[0][:, :, None] == want[0][:, None, :]) & (want[0][:, None, :] >= 0)
    return float(hit.any(dim=2).sum().item()) / max(1, int(want[2].clamp(max=k).sum().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 4, 1024])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--oversample", type=int, nargs="+", default=[1, 2, 4, 8])
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
    from sparse_rx import binary as bn
    if not torch.cuda.is_available():
        raise SystemExit("bench_binary.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "w") if args.log else None

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    emit(what="setup", device=torch.cuda.get_device_name(0), generator="gaussian mixture", centres=args.centres, sigma=args.sigma, seed=args.seed,
         dim=args.dim, reps=args.reps, warmup=args.warmup)
    for n in args.docs:
        emb, queries = mixture(torch, dev, n, max(args.nq), args.dim, args.centres, args.sigma, args.seed)
        f32 = sparse_rx.DenseF32Index(emb, device=dev)
        f16 = sparse_rx.DenseHalfIndex(emb, dtype="f16", device=dev)
        binary = sparse_rx.DenseBinaryIndex(emb, center="mean", device=dev)
        del emb
        torch.cuda.empty_cache()
        W = binary.words
        emit(what="index", n_docs=n, f32_bytes=int(f32.emb.numel()) * 4, f16_bytes=f16.device_bytes(), binary_bytes=binary.device_bytes())
        # the +-1 rows of the torch route, from the index's own codes
        codes = torch.from_numpy(binary.bits_to_host().view(np.uint8)).to(dev)
        shifts = torch.arange(8, device=dev, dtype=torch.uint8)
        pm_docs = torch.empty((n, 32 * W), dtype=torch.float16, device=dev)
        for lo in range(0, n, 1 << 20):
            b = (codes[lo: lo + (1 << 20), :, None] >> shifts) & 1
            pm_docs[lo: lo + (1 << 20)] = (b.reshape(b.shape[0], -1).to(torch.float16) * 2 - 1)
        del codes
        for nq in args.nq:
            q = queries[:nq].contiguous()
            qb = binary.encode_queries_device(q)
            bq = (qb.view(torch.uint8)[:, :, None] >> shifts) & 1
            pm_q = bq.reshape(nq, -1).to(torch.float16) * 2 - 1
            for k in args.k:
                pools = sorted({bn.screen_pool(k, o, n) for o in args.oversample})
                routes = {"exact_f32": lambda: f32.search_device(q, k), "exact_f16": lambda: f16.search_device(q, k)}
                screened = {o: bn.ScreenedDenseIndex(f32, binary, o) for o in args.oversample}
                for m in pools:
                    routes[f"hamming_m{m}"] = (lambda m=m: binary.hamming_search_device(None, m, q_bits=qb))
                for o, sc in screened.items():
                    routes[f"screened_f32_o{o}"] = (lambda sc=sc: sc.search_device(q, k))
                run_torch = nq * n <= args.torch_max_cells
                if run_torch:
                    m_t = pools[-1]
                    routes[f"torch_pm1_f16_m{m_t}"] = lambda: torch.topk(pm_q @ pm_docs.T, m_t, dim=1)
                    # the same top-m distance multisets (the ids inside the last tie class may differ: torch breaks ties its own way)
                    dot = torch.topk(pm_q @ pm_docs.T, m_t, dim=1).values.float()
                    want = ((32 * W - dot) / 2).to(torch.int32).sort(dim=1).values
                    got = binary.hamming_search_device(None, m_t, q_bits=qb)[1].sort(dim=1).values
                    assert torch.equal(got, want), "the Hamming search and the torch route disagree on the top-m distances"
                t = time_routes(torch, routes, args.reps, args.warmup)
                base = stats(t["exact_f32"])
                for name, ms in t.items():
                    row = dict(what="time", n_docs=n, dim=args.dim, nq=nq, k=k, route=name, **stats(ms))
                    row["speedup_vs_exact_f32"] = base["median_ms"] / row["median_ms"]
                    if name.startswith("hamming"):
                        sec = row["median_ms"] * 1e-3
                        if nq == 1:
                            row["code_bytes_per_s_over_8TBps"] = binary.device_bytes() / sec / PEAK_BYTES_PER_S
                        instr = 2 * W * ((n + 63) // 64) * nq  # one xor and one popcount per word, tile and query
                        row["xor_popcount_wave_instr"] = instr
                        row["issue_bound_ms"] = instr * 2 / (SIMDS * CLOCK_HZ) * 1e3
                        row["issue_bound_over_time"] = row["issue_bound_ms"] / row["median_ms"]
                    emit(**row)
                for o, sc in screened.items():  # is the gain beyond the two routes' combined run-to-run spread?
                    a, b = t["exact_f32"], t[f"screened_f32_o{o}"]
                    gain = float(np.median(a) - np.median(b))
                    spread = (max(a) - min(a)) + (max(b) - min(b))
                    emit(what="verdict", n_docs=n, nq=nq, k=k, oversample=o, gain_ms=gain, combined_spread_ms=float(spread),
                         screened_beats_exact_f32=bool(gain > spread))
                want = f32.search_device(q, k)
                for o, sc in screened.items():
                    emit(what="recall", n_docs=n, nq=nq, k=k, oversample=o, pool=sc.pool(k), recall_at_k=recall(torch, sc.search_device(q, k), want, k))
        del f32, f16, binary, pm_docs
        torch.cuda.empty_cache()
    if log:
        log.close()


if __name__ == "__main__":
    main()
