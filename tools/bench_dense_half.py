"""What the half-precision dense index costs next to the f32 index, on the same vectors in one session:

  a. ``srx_dense_search_f32`` (unchanged code: the baseline) at nq = 1, 32, 1 024;
  b. ``srx_dense_search_half`` for f16 and bf16 at the same batch sizes;
  c. the conversion of the whole corpus (``srx_dense_convert_half``, device tensor in, one launch);
  d. ``srx_dense_score_docs_half`` at m = 100 candidates per query, nq = 1 024,

each the median of hipEvent-timed calls after warm-up, same device tensors, same stream.  The f32 search at nq = 1 024 takes
a quarter of a second per call, so it gets fewer iterations (``--slow-iters``).  Every line goes to stdout and to ``--out``
(default ``profiles/dense_half.log``, rewritten by each run).

    python tools/bench_dense_half.py [--docs 1000000] [--dim 768] [--k 100] [--iters 20] [--warmup 3] [--slow-iters 3] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slow-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_half.log"))
    a = ap.parse_args()
    log = open(a.out, "w", encoding="utf-8")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(20251)
    emb = torch.randn((a.docs, a.dim), generator=g, device=dev, dtype=torch.float32)
    queries = torch.randn((1024, a.dim), generator=g, device=dev, dtype=torch.float32)
    say(f"# python tools/bench_dense_half.py: {a.docs} docs x {a.dim}, k = {a.k}; median (min .. max) ms after {a.warmup} warm-up calls, "
        f"hipEvents on the current stream; {torch.cuda.get_device_name(0)}")
    rows = []
    f32 = sparse_rx.DenseF32Index(emb)
    base = {}
    for nq in (1, 32, 1024):
        slow = nq == 1024
        base[nq] = timed(lambda: f32.search_device(queries[:nq], a.k), a.slow_iters if slow else a.iters, 1 if slow else a.warmup)
        rows.append((f"f32 search, nq = {nq}", base[nq], None))
    del f32
    torch.cuda.empty_cache()
    for dtype in ("f16", "bf16"):
        t = timed(lambda: sparse_rx.DenseHalfIndex(emb, dtype=dtype), 5, 1)  # includes the allocation and the flag read
        rows.append((f"{dtype} build from a device tensor (convert + flag read)", t, None))
        ix = sparse_rx.DenseHalfIndex(emb, dtype=dtype)
        for nq in (1, 32, 1024):
            t = timed(lambda: ix.search_device(queries[:nq], a.k), a.iters, a.warmup)
            rows.append((f"{dtype} search, nq = {nq}", t, base[nq][0] / t[0]))
        d, _, c = ix.search_device(queries, a.k)
        t = timed(lambda: ix.score_docs_device(queries, d, c), a.iters, a.warmup)
        rows.append((f"{dtype} score_docs, nq = 1024, m = {a.k}", t, None))
        del ix
        torch.cuda.empty_cache()
    for name, t, speedup in rows:
        tail = "" if speedup is None else f"   {speedup:7.1f} x the f32 search"
        say(f"{name:56s} {t[0]:10.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){tail}")
    log.close()


if __name__ == "__main__":
    main()
