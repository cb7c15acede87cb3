"""What expanding a query batch from its feedback docs costs, on a corpus of ``--docs`` docs x 30 terms:
``--queries`` queries of 4 terms, R = 10 feedback docs (the batch's own first pass), 10 expansion terms --

  1. ``srx_feedback_expand`` (two launches) from the resident forward index;
  2. the obvious torch route on the same GPU, up to the selection: padded gather of the rows, one ``torch.sort`` of (query, term)
     keys, segment sums by ``index_add_``, ``topk`` per query.  It does not merge with the query or build the CSR, and its sums run
     in another order, so the tool reports how many queries select the same term set instead of comparing bits;
  3. ``srx_search`` of the plain batch at k = 10 and at k = R, for scale;
  4. the second pass: ``srx_search`` of the expanded batch (longer queries, which the planner routes as it sees fit) at k = 10,

each the median of ``--iters`` hipEvent-timed repetitions after ``--warmup``, same device tensors, same stream.

    python tools/bench_feedback.py [--docs 1000000] [--queries 1024] [--iters 20] [--warmup 5] > profiles/feedback.log
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
from bench_filtered import timed  # noqa: E402

VOCAB, PER_DOC, TERMS, R, N_TERMS, K, SEED = 50_000, 30, 4, 10, 10, 10, 411


def line(name, t, note=""):
    print(f"{name:72s} {t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){note}", flush=True)


def torch_select(fwd, gain, fb_doc, fb_score, L, n_terms):
    """The selection in torch ops (every position used): -> the selected term ids i64[nq, n_terms] (-1: none)"""
    nq, r = fb_doc.shape
    dev = fb_doc.device
    d = fb_doc.long() - fwd.doc_base
    a = fb_score / fb_score.sum(dim=1, keepdim=True)
    start = fwd.row_ptr[d]
    length = (fwd.row_ptr[d + 1] - start).clamp(max=L)
    j = torch.arange(L, device=dev)
    at = (start.unsqueeze(-1) + j).clamp(max=fwd.term.numel() - 1)
    valid = j < length.unsqueeze(-1)
    t = fwd.term[at].long()
    c = torch.where(valid, a.unsqueeze(-1) * (fwd.value[at] / fwd.doc_len[d].unsqueeze(-1)), torch.zeros((), device=dev))
    key = torch.arange(nq, device=dev).view(nq, 1, 1) * fwd.vocab + t
    key = torch.where(valid, key, torch.full((), nq * fwd.vocab, dtype=torch.int64, device=dev)).flatten()
    sk, order = torch.sort(key)
    new = torch.ones_like(sk, dtype=torch.bool)
    new[1:] = sk[1:] != sk[:-1]
    seg = new.cumsum(0) - 1
    seg_key = sk[new]
    fb = torch.zeros(seg_key.numel(), dtype=torch.float32, device=dev).index_add_(0, seg, c.flatten()[order])
    q_of, t_of = seg_key // fwd.vocab, seg_key % fwd.vocab
    live = q_of < nq
    first = torch.searchsorted(q_of, torch.arange(nq, device=dev))
    col = torch.arange(seg_key.numel(), device=dev) - first[q_of.clamp(max=nq - 1)]
    score = torch.full((nq, r * L), -1.0, dtype=torch.float32, device=dev)
    terms = torch.full((nq, r * L), -1, dtype=torch.int64, device=dev)
    score[q_of[live], col[live]] = fb[live] * gain[t_of[live]]
    terms[q_of[live], col[live]] = t_of[live]
    top = torch.topk(score, n_terms, dim=1)
    return torch.where(top.values > 0, terms.gather(1, top.indices), torch.full((), -1, dtype=torch.int64, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, cols, tf, dl = synth.uniform_chunk_torch(0, a.docs, VOCAB, PER_DOC, SEED, dev)
    df = torch.bincount(cols, minlength=VOCAB).cpu().numpy()
    idf = torch.as_tensor(np.log((a.docs - df + 0.5) / (df + 0.5)).astype(np.float32), device=dev)
    ix = sparse_rx.DeviceIndex.from_coo(rows, cols, tf, idf, a.docs, doc_lengths=dl, k1=1.2, b=0.75, avgdl=float(dl.mean().item()), device=dev)
    if ix.post is not None:
        ix.drop_canonical()
    o = torch.sort(rows, stable=True).indices
    indptr = torch.zeros(a.docs + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.bincount(rows.long(), minlength=a.docs).cumsum(0)
    fwd = sparse_rx.ForwardIndex.from_csr(indptr, cols[o], tf[o], idf, doc_lengths=dl, device=dev)
    del rows, cols, tf, o
    gain = idf.clamp(min=0.0)
    q = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in synth.queries_np(a.queries, VOCAB, TERMS, seed=SEED + 1)]
    L = fwd.default_row_cap(R)
    print(f"# {a.docs} docs x {PER_DOC} draws of {VOCAB} terms (forward index {fwd.device_bytes() / 2 ** 20:.0f} MiB next to the {ix.device_bytes() / 2 ** 20:.0f} MiB "
          f"index, longest row {fwd.max_row_terms}), {a.queries} queries x {TERMS} terms, R = {R}, row_cap = {L}, {N_TERMS} expansion terms; median (min .. max) ms "
          f"of {a.iters} repetitions after {a.warmup} warm-up, hipEvents on the current stream; {torch.cuda.get_device_name(0)}", flush=True)
    d, s, c = ix.search_device(*q, R)
    torch.cuda.synchronize()
    full = int((c == R).sum())
    kw = dict(fb_docs=R, n_terms=N_TERMS, alpha=0.5, beta=0.5, term_gain=gain)
    out = fwd.expand_device(*q, d, s, c, **kw)
    t_exp = timed(lambda: fwd.expand_device(*q, d, s, c, out=out, **kw), a.iters, a.warmup)
    t_tor = timed(lambda: torch_select(fwd, gain, d, s, L, N_TERMS), a.iters, a.warmup)
    line("srx_feedback_expand: gather, sort, sums, selection, merge, CSR", t_exp)
    line("torch ops on the same GPU: gather, sort, index_add_, topk (no merge, no CSR)", t_tor,
         f"   kernel path is {t_tor[0] / t_exp[0]:.1f}x faster (spreads: kernels {t_exp[2] - t_exp[1]:.3f} ms, torch {t_tor[2] - t_tor[1]:.3f} ms; "
         f"difference {t_tor[0] - t_exp[0]:.3f} ms)")
    # same selection?  beta alone: the row is the selected terms
    sel = fwd.expand_device(*q, d, s, c, fb_docs=R, n_terms=N_TERMS, alpha=0.0, beta=1.0, term_gain=gain)
    picked = torch_select(fwd, gain, d, s, L, N_TERMS)
    torch.cuda.synchronize()
    p, t = sel[0].cpu().numpy(), sel[1].cpu().numpy()
    picked = picked.cpu().numpy()
    same = sum(set(t[p[i]: p[i + 1]].tolist()) == set(x for x in picked[i].tolist() if x >= 0) for i in range(a.queries))
    print(f"# {full} of {a.queries} first-pass lists hold {R} docs; {same} of {a.queries} queries select the same term set on both routes (sums in another order "
          f"and ties may differ)", flush=True)
    lens = np.diff(out[0].cpu().numpy())
    line(f"srx_search, plain batch, k = {K}", timed(lambda: ix.search_device(*q, K), a.iters, a.warmup))
    line(f"srx_search, plain batch, k = {R} (the first pass)", timed(lambda: ix.search_device(*q, R), a.iters, a.warmup))
    line(f"srx_search, expanded batch, k = {K} (the second pass)", timed(lambda: ix.search_device(out[0], out[1], out[2], K), a.iters, a.warmup),
         f"   rows of {lens.min()} .. {lens.max()} terms, mean {lens.mean():.1f}")
    line("both passes and the expansion, one call after the other", timed(
        lambda: ix.search_device(*fwd.expand_device(*q, *ix.search_device(*q, R), out=out, **kw)[:3], K), a.iters, a.warmup))
    ix.close()
    fwd.close()


if __name__ == "__main__":
    main()
