"""What boosting ranked lists by field values costs:

  1. the kernel: ``srx_boost_topk`` for 1 024 lists of m in {128, 1 024, 2 048} random docs of a 10 M-doc table, k = 10 and k = m / 2,
     with one clause (a gauss decay over an int64 date) and with four (int64, int32, float32, int64), score_mode and boost_mode
     "multiply" -- against the same step written in torch ops on the same GPU: gather the values, the same arithmetic as separate
     float32 ops, ``topk``.  The tool asserts that both routes give equal score bits;
  2. the exact paged door: ``boost_deep`` (search, boost, page on) for ``--queries`` queries, k = 10, against the plain search of
     the same batch on the corpus of ``--corpus``, for a gauss decay at two scales, with the search calls per batch, the cost of
     the search at the depths the door asks for, and the rows each query has to read before the stop rule holds,

each the median of ``--iters`` hipEvent-timed repetitions after ``--warmup``, same device tensors, same stream.

    python tools/bench_boost.py [--corpus uniform100k|c3] [--queries 1000] [--iters 20] [--warmup 5] [--no-search] > profiles/boost.log
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparse_rx  # noqa: E402
from sparse_rx import synth  # noqa: E402
from sparse_rx.boost import BoostFn, BoostResolver, boost_deep  # noqa: E402
from bench_filtered import build, timed  # noqa: E402

N_TABLE, NQ = 10_000_000, 1024
DAY = 86400


def line(name, t, note=""):
    print(f"{name:72s} {t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){note}", flush=True)


def torch_boost(tensors, res, knots, doc, score, k):
    """The same step in torch ops (every position live, every doc with a value): gather, the header's arithmetic as separate float32
    ops, multiply, topk"""
    local = doc.long()
    F = None
    for c in res.clauses:
        data = tensors[res.names[int(c["col"])]]
        v = data[local]
        if data.dtype == torch.float32:
            x = v - float(np.asarray([int(c["origin"]) & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
        else:
            x = (v.double() - float(int(c["origin"]))).float()
        if int(c["flags"]) & 1:
            x = x.abs()
        t = x * float(c["inv_step"])
        k0, n_seg = int(c["knot0"]), int(c["n_seg"])
        i = t.clamp(0, n_seg - 1).long()  # truncation; the clamps keep the gathers of the two outer branches inside the table
        fr = t - i.float()
        y0, y1 = knots[k0 + i], knots[k0 + i + 1]
        f = y0 + fr * (y1 - y0)
        f = torch.where(t > 0, torch.where(t >= n_seg, knots[k0 + n_seg], f), knots[k0])
        g = float(c["weight"]) * f
        F = g if F is None else F * g
    val, idx = torch.topk(score * F, k, dim=1)
    return doc.gather(1, idx), val


def rows_needed(ix, fn, q, k, f_hi, step=32, limit=8192):
    """Per query, the rows of its ranking read (in pages of ``step``) when the door's stop rule first holds under "multiply": what
    the data asks for, as opposed to what pages of 1 024 read"""
    d, s, c = ix.search_device(*q, step)
    kd, ks, kc = fn(d, s, c, k)
    need = torch.full((d.shape[0],), -1, dtype=torch.int64, device=d.device)
    depth = step
    while True:
        settled = ((kc == k) & (s[:, -1] * f_hi < ks[:, k - 1])) | (c < step)
        need = torch.where((need < 0) & settled, torch.full_like(need, depth), need)
        if bool((need >= 0).all()) or depth >= limit:
            return torch.where(need < 0, torch.full_like(need, limit), need)
        d, s, c = ix.search_device(*q, step, after=(d[:, -1].contiguous(), s[:, -1].contiguous()))
        kd, ks, kc = fn(d, s, c, k, carry=(kd, ks, kc))
        depth += step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="uniform100k", choices=["uniform100k", "c3"])
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-search", action="store_true", help="skip part 2 (it builds the sparse index of the corpus)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    now = 1_700_000_000
    cols = {"date": now - rng.integers(0, 720 * DAY, N_TABLE).astype(np.int64), "votes": rng.integers(0, 10_000, N_TABLE).astype(np.int32),
            "price": (rng.random(N_TABLE) * 200).astype(np.float32), "edited": now - rng.integers(0, 90 * DAY, N_TABLE).astype(np.int64)}
    table = sparse_rx.FieldTable.from_columns(cols, device=dev)
    tensors = {n: torch.as_tensor(v, device=dev) for n, v in cols.items()}
    one = {"functions": [{"decay": {"field": "date", "origin": now, "scale": 30 * DAY, "kind": "gauss"}}]}
    four = {"functions": one["functions"] + [{"field_value": {"field": "votes", "lo": 0, "hi": 10_000, "modifier": "log1p", "factor": 0.01}},
                                             {"decay": {"field": "price", "origin": 50.0, "scale": 25.0, "kind": "linear", "offset": 5.0}},
                                             {"decay": {"field": "edited", "origin": now, "scale": 7 * DAY, "kind": "exp", "weight": 1.5}}]}
    print(f"# {NQ} lists of random docs of a {N_TABLE}-doc table, four columns ({table.device_bytes() / 2 ** 20:.0f} MiB resident); median (min .. max) ms "
          f"of {a.iters} repetitions after {a.warmup} warm-up, hipEvents on the current stream; {torch.cuda.get_device_name(0)}", flush=True)
    for name, spec in (("1 clause ", one), ("4 clauses", four)):
        res = BoostResolver(table.columns, spec)
        fn = BoostFn(table, res)
        for m in (128, 1024, 2048):
            doc = torch.as_tensor(rng.integers(0, N_TABLE, (NQ, m)).astype(np.int32), device=dev)
            score = torch.as_tensor((rng.random((NQ, m)) * 20 + 0.1).astype(np.float32), device=dev)
            for k in (10, m // 2):
                t = timed(lambda: fn(doc, score, None, k), a.iters, a.warmup)
                tt = timed(lambda: torch_boost(tensors, res, fn.knots, doc, score, k), a.iters, a.warmup)
                got, exp = fn(doc, score, None, k), torch_boost(tensors, res, fn.knots, doc, score, k)
                torch.cuda.synchronize()
                assert torch.equal(got[1].view(torch.int32), exp[1].view(torch.int32)), "the torch restatement and the kernel disagree"
                line(f"{name}, m = {m:4d}, k = {k:4d}: srx_boost_topk", t)
                line(f"{name}, m = {m:4d}, k = {k:4d}: torch ops on the same GPU", tt,
                     f"   kernel is {tt[0] / t[0]:.1f}x faster (spreads: kernel {t[2] - t[1]:.3f} ms, torch {tt[2] - tt[1]:.3f} ms; "
                     f"difference {tt[0] - t[0]:.3f} ms)")
    table.close()
    del tensors
    if a.no_search:
        return
    # ---- the exact paged door against the plain search
    ix, V, terms, qseed = build(a.corpus, dev)
    if ix.post is not None:
        ix.drop_canonical()
    q = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in synth.queries_np(a.queries, V, terms, seed=qseed)]
    date = now - rng.integers(0, 720 * DAY, ix.n_docs).astype(np.int64)
    table = sparse_rx.FieldTable.from_columns({"date": date}, device=dev, doc_base=ix.doc_base)
    k, first = 10, 64
    calls = []

    def search_fn(qp, qt, qw, kk, after=None):
        calls.append(kk)
        return ix.search_device(qp, qt, qw, kk, after=after)

    line(f"{a.corpus}: {a.queries} queries x {terms} terms, k = {k}: plain search", timed(lambda: ix.search_device(*q, k), a.iters, a.warmup))
    line(f"{a.corpus}: plain search, k = {first} (the door's first fetch)", timed(lambda: ix.search_device(*q, first), a.iters, a.warmup))
    for kk in (128, 1024):  # what a further page costs: the door's time is its search calls
        line(f"{a.corpus}: plain search, k = {kk}", timed(lambda: ix.search_device(*q, kk), a.iters, a.warmup))
    for scale_days in (360, 30):
        res = BoostResolver(table.columns, {"functions": [{"decay": {"field": "date", "origin": now, "scale": scale_days * DAY, "kind": "gauss"}}]})
        fn = BoostFn(table, res)
        door = lambda: boost_deep(search_fn, fn, *q, k, first, page=1024)
        del calls[:]
        out = door()
        n_calls, rows = len(calls), sum(calls)
        line(f"{a.corpus}: gauss decay, scale {scale_days} days of 720: the exact door", timed(door, a.iters, a.warmup),
             f"   {n_calls} search call(s), {rows} rows per query slot read, {int((out[2] == k).sum())} of {a.queries} queries full")
        need = rows_needed(ix, fn, q, k, float(res.F_hi)).cpu().numpy()
        print(f"{'':72s} rows a query must read before it settles (pages of 32): median {np.median(need):.0f}, p90 {np.percentile(need, 90):.0f}, "
              f"p99 {np.percentile(need, 99):.0f}, max {need.max()}", flush=True)
    ix.close()
    table.close()


if __name__ == "__main__":
    main()
