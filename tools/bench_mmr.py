"""What the MMR selection costs, next to what a user could do before it without leaving the device, on the same
vectors in one session:

  a. ``mmr_device`` of ``DenseHalfIndex`` (f16, bf16) and ``DenseF32Index``: one Gram launch + one selection launch per call;
  b. the same call at ``k = 1`` -- the Gram stage and a single selection step -- so that the difference to (a) is what the
     remaining ``k - 1`` steps cost (the two kernels' own durations come from ``rocprofv3 --kernel-trace --stats`` in a run of
     its own: ``--engine-only`` keeps that run short);
  c. the baseline, a torch restatement on the same GPU: a row gather from a row-major tensor of the same type, ``torch.bmm``,
     the cosine normalisation and a ``k``-step loop of torch ops (arg-max, scatter, gather, maximum).  Its picks are compared
     with the engine's: the share of (query, step) pairs that agree is printed (its arithmetic is not the engine's to the bit,
     so near-ties may go the other way).

Pools are ``m`` distinct random docs per query -- no locality between a pool's rows, the worst case for the gather -- with
random positive relevances.  Each figure is the median of hipEvent-timed calls after warm-up, same tensors, same stream.  Every
line goes to stdout and to ``--out`` (default ``profiles/mmr.log``, rewritten by each run).  Run it under a time limit and
check its exit status, e.g. ``timeout -k 10 900 python tools/bench_mmr.py``.

    python tools/bench_mmr.py [--docs 1000000] [--dim 768] [--nq 1024] [--m 128] [--k 10] [--lam 0.5] [--iters 20] [--warmup 3]
                              [--engine-only] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparse_rx  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def torch_mmr(table, rows, rel, k, lam):
    """The baseline: cosine MMR in torch ops on the device.  table [n, dim] row-major, rows i64[nq, m], rel f32[nq, m]."""
    x = table[rows]                                        # the gather: [nq, m, dim]
    g = torch.bmm(x, x.transpose(1, 2)).float()            # [nq, m, m]
    n = g.diagonal(dim1=1, dim2=2).clamp_min(0).sqrt()
    d = n[:, :, None] * n[:, None, :]
    s = torch.where(d > 0, g / d, torch.zeros_like(g))
    wr = lam * rel
    pen = torch.zeros_like(rel)
    is_open = torch.ones_like(rel, dtype=torch.bool)
    picks = []
    for t in range(k):
        v = wr if t == 0 else wr - (1.0 - lam) * pen
        best = v.masked_fill(~is_open, float("-inf")).argmax(dim=1)
        picks.append(best)
        is_open.scatter_(1, best[:, None], False)
        col = s.gather(2, best[:, None, None].expand(-1, s.shape[1], 1)).squeeze(2)  # S(c, picked)
        pen = col if t == 0 else torch.maximum(pen, col)
    return torch.stack(picks, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--engine-only", action="store_true", help="only the engine's calls (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr.log"))
    a = ap.parse_args()
    log = open(a.out, "w", encoding="utf-8")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(20252)
    emb = torch.randn((a.docs, a.dim), generator=g, device=dev, dtype=torch.float32)
    rows = torch.stack([torch.randperm(a.docs, generator=g, device=dev)[: a.m] for _ in range(a.nq)])  # distinct per query
    cand_doc = rows.to(torch.int32)
    cand_rel = torch.rand((a.nq, a.m), generator=g, device=dev, dtype=torch.float32) + 0.5
    say(f"# python tools/bench_mmr.py: {a.docs} docs x {a.dim}, {a.nq} queries, pool m = {a.m}, k = {a.k}, cosine, lambda = {a.lam}; median "
        f"(min .. max) ms after {a.warmup} warm-up calls, hipEvents on the current stream; {torch.cuda.get_device_name(0)}")
    out = []
    for storage in ("f16", "bf16", "f32"):
        if storage == "f32":
            ix, table = sparse_rx.DenseF32Index(emb), emb
        else:
            ix = sparse_rx.DenseHalfIndex(emb, dtype=storage)
            table = emb.to(torch.float16 if storage == "f16" else torch.bfloat16)  # what a user would keep: row-major, the same type
        call = lambda k: ix.mmr_device(cand_doc, cand_rel, None, k, a.lam, "cosine")
        full = timed(lambda: call(a.k), a.iters, a.warmup)
        one = timed(lambda: call(1), a.iters, a.warmup)
        out.append((f"{storage} engine, k = {a.k} (Gram + selection, two launches)", full, None))
        out.append((f"{storage} engine, k = 1 (Gram + one step)", one, None))
        out.append((f"{storage} engine, steps 2 .. {a.k} (the difference)", (full[0] - one[0], 0.0, 0.0), None))
        if not a.engine_only:
            base = timed(lambda: torch_mmr(table, rows, cand_rel, a.k, a.lam), a.iters, a.warmup)
            def gather_bmm():
                x = table[rows]
                return torch.bmm(x, x.transpose(1, 2))

            gram = timed(gather_bmm, a.iters, a.warmup)
            out.append((f"{storage} torch baseline (gather + bmm + {a.k}-step loop)", base, base[0] / full[0]))
            out.append((f"{storage} torch gather + bmm alone", gram, None))
            doc = call(a.k)[0]
            picks = torch.gather(cand_doc, 1, torch_mmr(table, rows, cand_rel, a.k, a.lam))
            agree = float((doc == picks).float().mean().item())
            out.append((f"{storage} picks equal to the baseline's: {100 * agree:.2f} % of {a.nq * a.k}", None, None))
        del ix, table
        torch.cuda.empty_cache()
    for name, t, ratio in out:
        if t is None:
            say(name)
            continue
        tail = "" if ratio is None else f"   = {ratio:6.2f} x the engine's call"
        say(f"{name:62s} {t[0]:10.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){tail}")
    log.close()


if __name__ == "__main__":
    main()
