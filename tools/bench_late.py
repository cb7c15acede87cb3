"""What the late-interaction rerank costs, next to what a user could do before it without leaving the device, on
the same vectors in one session:

  a. ``TokenIndex.rerank_device`` (pack + score + rank launches) and ``TokenIndex.score_docs_device`` (pack + score);
  b. the baseline, a torch restatement on the same GPU: a padded gather of every candidate's token rows from a row-major half
     tensor (docs padded to the longest doc of the corpus, a zero row behind the store for the padding), a batched matmul with
     the query tokens, a masked ``amax`` over the doc tokens, a sum over the query tokens and ``topk``; run in query chunks
     that keep the gathered block within ``--chunk-mb``.  Its arithmetic is not the engine's to the bit, so near-ties may
     go the other way: the share of queries whose top-k SETS agree is printed.

Pools are ``m`` distinct random docs per query -- no locality between a pool's docs, the worst case for the gather.  Token
counts are drawn from a normal distribution around ``--tokens`` (a quarter of it as deviation, clipped to 1 .. 2 x).  Each
figure is the median of hipEvent-timed calls after warm-up, same tensors, same stream; min .. max is the run-to-run spread.
The gathered token bytes (the token rows of every candidate of every query, once) per second are printed as a fraction of
8 TB/s.  Every line goes to stdout and to ``--out`` (default ``profiles/late_interaction.log``, rewritten by each run).  Run
it under a time limit and check its exit status, e.g. ``timeout -k 10 900 python tools/bench_late.py``.

    python tools/bench_late.py [--docs 200000] [--tokens 80] [--dim 128] [--dtype f16] [--nq 1024] [--tq 32] [--m 128] [--k 10]
                               [--iters 20] [--warmup 3] [--chunk-mb 1024] [--engine-only] [--out FILE]
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


def torch_maxsim(table, tok_ptr, t_max, q_half, rows, k, chunk):
    """The baseline.  table [n_tok + 1, dim] row-major half (the last row zeros), tok_ptr i64[n_docs + 1], q_half
    [nq, tq, dim], rows i64[nq, m].  Returns (scores f32[nq, m], top-k positions i64[nq, k])."""
    n_tok = table.shape[0] - 1
    t = torch.arange(t_max, device=table.device)
    scores = []
    for lo in range(0, rows.shape[0], chunk):
        r = rows[lo: lo + chunk]
        start, count = tok_ptr[r], tok_ptr[r + 1] - tok_ptr[r]                # [b, m]
        live = t[None, None, :] < count[:, :, None]                             # [b, m, t_max]
        idx = torch.where(live, start[:, :, None] + t[None, None, :], n_tok)
        x = table[idx]                                                          # the padded gather: [b, m, t_max, dim]
        sim = torch.matmul(q_half[lo: lo + chunk, None], x.transpose(2, 3))    # [b, m, tq, t_max]
        sim = sim.float().masked_fill(~live[:, :, None, :], float("-inf"))
        scores.append(sim.amax(dim=3).sum(dim=2))
    s = torch.cat(scores)
    return s, s.topk(k, dim=1).indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--tokens", type=int, default=80)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--tq", type=int, default=32)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk-mb", type=int, default=1024, help="gathered block of one baseline chunk")
    ap.add_argument("--engine-only", action="store_true", help="only the engine's calls (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "late_interaction.log"))
    a = ap.parse_args()
    log = open(a.out, "w", encoding="utf-8")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(20254)
    counts = (torch.randn(a.docs, generator=g, device=dev) * (a.tokens / 4) + a.tokens).round().clamp(1, 2 * a.tokens).to(torch.int64)
    tok_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), counts.cumsum(0)])
    n_tok, t_max = int(tok_ptr[-1].item()), int(counts.max().item())
    tok = torch.randn((n_tok, a.dim), generator=g, device=dev, dtype=torch.float32)
    q_tok = torch.randn((a.nq, a.tq, a.dim), generator=g, device=dev, dtype=torch.float32)
    rows = torch.stack([torch.randperm(a.docs, generator=g, device=dev)[: a.m] for _ in range(a.nq)])  # distinct per query
    cand_doc = rows.to(torch.int32)
    ix = sparse_rx.TokenIndex.from_token_embeddings(tok, counts.cpu().numpy(), dtype=a.dtype, device="cuda:0")
    half = torch.float16 if a.dtype == "f16" else torch.bfloat16
    gathered = int(counts[rows].sum().item()) * ix.dim_pad * 2
    say(f"# python tools/bench_late.py: {a.docs} docs, {n_tok} token rows x {a.dim} ({a.dtype}; {t_max} in the longest doc), {a.nq} queries x "
        f"{a.tq} tokens, pool m = {a.m}, k = {a.k}; median (min .. max) ms after {a.warmup} warm-up calls, hipEvents on the current "
        f"stream; {torch.cuda.get_device_name(0)}")
    say(f"# token rows gathered per call: {gathered / 1e9:.3f} GB")
    out = []
    rer = timed(lambda: ix.rerank_device(q_tok, None, cand_doc, None, a.k), a.iters, a.warmup)
    sco = timed(lambda: ix.score_docs_device(q_tok, None, cand_doc), a.iters, a.warmup)
    out.append((f"engine rerank (pack + score + rank, k = {a.k})", rer, None))
    out.append(("engine score_docs (pack + score)", sco, None))
    if not a.engine_only:
        table = torch.cat([tok.to(half), torch.zeros((1, a.dim), dtype=half, device=dev)])  # what a user would keep: row-major, the same type
        del tok
        torch.cuda.empty_cache()
        q_half = q_tok.to(half)
        chunk = max(1, (a.chunk_mb << 20) // (a.m * t_max * a.dim * 2))
        base = timed(lambda: torch_maxsim(table, tok_ptr, t_max, q_half, rows, a.k, chunk), a.iters, a.warmup)
        out.append((f"torch baseline (padded gather + matmul + masked amax + sum + topk, {chunk} queries per chunk)", base, base[0] / rer[0]))
        doc, _, _ = ix.rerank_device(q_tok, None, cand_doc, None, a.k)
        picks = torch.gather(cand_doc, 1, torch_maxsim(table, tok_ptr, t_max, q_half, rows, a.k, chunk)[1])
        same = (doc.sort(dim=1).values == picks.sort(dim=1).values).all(dim=1).float().mean().item()
        out.append((f"queries whose top-{a.k} SET equals the baseline's: {100 * same:.2f} % of {a.nq}", None, None))
    for name, t, ratio in out:
        if t is None:
            say(name)
            continue
        tail = "" if ratio is None else f"   = {ratio:6.2f} x the engine's rerank"
        say(f"{name:100s} {t[0]:10.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){tail}")
    for name, t in (("rerank", rer), ("score_docs", sco)):
        rate = gathered / (t[0] * 1e-3)
        say(f"engine {name}: {rate / 1e12:.3f} TB/s of gathered token rows = {100 * rate / 8e12:.1f} % of 8 TB/s")
    log.close()


if __name__ == "__main__":
    main()
