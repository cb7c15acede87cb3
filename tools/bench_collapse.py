"""What collapsing ranked lists by a field costs:

  1. the kernel: ``srx_collapse_topk`` for 1 024 lists of m in {128, 1 024, 2 048} random docs of a 10 M-doc table, k in {10, 100},
     per_group in {1, 3}, by an int64 column with about 8 docs per key -- against the same step written in torch ops on the same
     GPU: gather the keys, stable sort by key per row, rank within the segment, mask, compact.  The tool asserts that both routes
     give equal bits (docs, score bits, counts);
  2. the exact paged door: ``collapse_deep`` (search, collapse, page on) for ``--queries`` queries, k = 10, against the plain search
     of the same batch, on the corpus of ``--corpus``,

each the median of ``--iters`` hipEvent-timed repetitions after ``--warmup``, same device tensors, same stream.

    python tools/bench_collapse.py [--corpus uniform100k|c3] [--queries 1000] [--iters 20] [--warmup 5] [--no-search] > profiles/collapse.log
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
from sparse_rx.backend import collapse_deep  # noqa: E402
from bench_filtered import build, timed  # noqa: E402

N_TABLE, DOCS_PER_KEY, NQ = 10_000_000, 8, 1024


def line(name, t, note=""):
    print(f"{name:64s} {t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){note}", flush=True)


def torch_collapse(keys, doc, score, k, per_group):
    """The same step in torch ops (every position live, every doc with a key): gather, stable sort by key per row, rank within the
    segment, mask, compact"""
    nq, m = doc.shape
    dev = doc.device
    kk = keys[doc.long()]
    sk, order = torch.sort(kk, dim=1, stable=True)
    idx = torch.arange(m, device=dev).expand(nq, m)
    new = torch.ones((nq, m), dtype=torch.bool, device=dev)
    new[:, 1:] = sk[:, 1:] != sk[:, :-1]
    start = torch.where(new, idx, torch.zeros_like(idx)).cummax(dim=1).values
    rank = torch.empty_like(idx).scatter_(1, order, idx - start)  # back in list order: the stable sort kept it inside a segment
    keep = rank < per_group
    place = keep.cumsum(dim=1) - 1
    sel = keep & (place < k)
    out_doc = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    out_score = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    rows = torch.arange(nq, device=dev).unsqueeze(1).expand(nq, m)[sel]
    out_doc[rows, place[sel]] = doc[sel]
    out_score[rows, place[sel]] = score[sel]
    return out_doc, out_score, keep.sum(dim=1).clamp(max=k).to(torch.int32)


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
    keys = rng.integers(0, N_TABLE // DOCS_PER_KEY, N_TABLE, dtype=np.int64) << 8  # keys that do not fit 32 bits
    table = sparse_rx.FieldTable.from_columns({"parent": keys}, device=dev)
    d_keys = torch.as_tensor(keys, device=dev)
    print(f"# {NQ} lists of random docs of a {N_TABLE}-doc table, int64 column ({table.device_bytes() / 2 ** 20:.0f} MiB resident), about {DOCS_PER_KEY} docs per "
          f"key; median (min .. max) ms of {a.iters} repetitions after {a.warmup} warm-up, hipEvents on the current stream; {torch.cuda.get_device_name(0)}",
          flush=True)
    for m in (128, 1024, 2048):
        doc = torch.as_tensor(rng.integers(0, N_TABLE, (NQ, m)).astype(np.int32), device=dev)
        score = torch.as_tensor(rng.standard_normal((NQ, m)).astype(np.float32), device=dev)
        for k in (10, 100):
            for per_group in (1, 3):
                t = timed(lambda: table.collapse_device("parent", doc, score, None, k, per_group), a.iters, a.warmup)
                tt = timed(lambda: torch_collapse(d_keys, doc, score, k, per_group), a.iters, a.warmup)
                got = table.collapse_device("parent", doc, score, None, k, per_group)
                exp = torch_collapse(d_keys, doc, score, k, per_group)
                torch.cuda.synchronize()
                for g, e in zip(got, exp):
                    assert torch.equal(g.view(torch.int32), e.view(torch.int32)), "the torch restatement and the kernel disagree"
                line(f"m = {m:4d}, k = {k:3d}, per_group = {per_group}: srx_collapse_topk", t)
                line(f"m = {m:4d}, k = {k:3d}, per_group = {per_group}: torch ops on the same GPU", tt,
                     f"   kernel is {tt[0] / t[0]:.1f}x faster (spreads: kernel {t[2] - t[1]:.3f} ms, torch {tt[2] - tt[1]:.3f} ms; "
                     f"difference {tt[0] - t[0]:.3f} ms)")
    table.close()
    del d_keys
    if a.no_search:
        return
    # ---- the exact paged door against the plain search
    ix, V, terms, qseed = build(a.corpus, dev)
    if ix.post is not None:
        ix.drop_canonical()
    q = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in synth.queries_np(a.queries, V, terms, seed=qseed)]
    parent = (rng.permutation(ix.n_docs) // DOCS_PER_KEY).astype(np.int64)
    table = sparse_rx.FieldTable.from_columns({"parent": parent}, device=dev, doc_base=ix.doc_base)
    k, first = 10, 64
    calls = []

    def search_fn(qp, qt, qw, kk, after=None):
        calls.append(kk)
        return ix.search_device(qp, qt, qw, kk, after=after)

    for per_group in (1, 3):
        collapse_fn = lambda d, s, c, kk: table.collapse_device("parent", d, s, c, kk, per_group)
        door = lambda: collapse_deep(search_fn, collapse_fn, *q, k, first, page=1024)
        del calls[:]
        out = door()
        n_calls = len(calls)
        line(f"{a.corpus}: {a.queries} queries x {terms} terms, k = {k}: plain search", timed(lambda: ix.search_device(*q, k), a.iters, a.warmup))
        line(f"{a.corpus}: plain search, k = {first} (the door's first fetch)", timed(lambda: ix.search_device(*q, first), a.iters, a.warmup))
        line(f"{a.corpus}: collapse_by parent, per_group = {per_group}: the exact door", timed(door, a.iters, a.warmup),
             f"   {n_calls} search call(s) per batch, {int((out[2] == k).sum())} of {a.queries} queries full")
    ix.close()
    table.close()


if __name__ == "__main__":
    main()
