"""What evaluating ranked lists on the GPU costs:

``srx_eval_lists`` (per-query metrics at 4 cutoffs AND their means: three launches) for 1 024 and 65 536 lists of m in {128, 1 024,
2 048} docs against judgment rows of 16, 256 and 4 096 docs -- against ONE batched route written in torch ops on the same GPU:
``searchsorted`` of offset-keyed candidates into offset-keyed judgments, ``cumsum`` along the list, masked sums, ``mean``.  1 024 lists
have a row each; 65 536 lists are 64 rankings for each of 1 024 judged queries (the model-selection shape).  A third of every list's
positions are docs of its row.  The tool asserts that both routes give EQUAL integer outputs (hits, judged, R) and prints the
largest difference of the float outputs (torch's cumsum does not add in the contract's order).

Each figure is the median (min .. max) of ``--iters`` hipEvent-timed repetitions after ``--warmup``, same device tensors, same stream.

    python tools/bench_eval.py [--iters 20] [--warmup 5] [--small] > profiles/eval.log
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
from sparse_rx import evaluate as ev  # noqa: E402
from bench_filtered import timed  # noqa: E402

N_DOCS, N_GAIN, REL_LEVEL = 10_000_000, 5, 1
KS = (10, 100, 1000, 2048)
STRIDE = 1 << 32  # row * STRIDE + doc: one sorted int64 key per judgment


def line(name, t, note=""):
    print(f"{name:72s} {t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){note}", flush=True)


def make_rows(gen, n_rows, row_len, dev):
    """n_rows rows of row_len judged docs each, strictly ascending, grades 0 .. 4 (half of them 0), as device tensors [n_rows, row_len]"""
    doc = torch.sort(torch.randint(0, N_DOCS - row_len, (n_rows, row_len), generator=gen, device=dev), dim=1).values + torch.arange(row_len, device=dev)
    grade = torch.randint(0, N_GAIN, (n_rows, row_len), generator=gen, device=dev) * (torch.rand((n_rows, row_len), generator=gen, device=dev) < 0.5)
    ideal = torch.sort(grade, dim=1, descending=True).values
    return doc.int(), grade.int(), ideal.int()


def torch_eval(key_j, grade_flat, ideal, rel_rows, gain, discount, doc, q_rows, ks):
    """The same metrics in batched torch ops: -> (out f32[nq, n_k, 8], hits, judged i32[nq, n_k], R i32[nq], mean f64[n_k, 8])"""
    nq, m = doc.shape
    rows = q_rows.long()
    key_c = rows[:, None] * STRIDE + doc.long()
    pos = torch.searchsorted(key_j, key_c).clamp_(max=key_j.numel() - 1)
    found = key_j[pos] == key_c
    g = torch.where(found, grade_flat[pos], 0).clamp_(0, N_GAIN - 1)
    rel = found & (g >= REL_LEVEL)
    rank = torch.arange(1, m + 1, device=doc.device, dtype=torch.float32)
    hits_cum, judged_cum = torch.cumsum(rel, 1), torch.cumsum(found, 1)
    dcg_cum = torch.cumsum(gain[g] * discount[None, :], 1)
    ap_cum = torch.cumsum(torch.where(rel, hits_cum.float() / rank[None, :], 0.0), 1)
    first = torch.where(rel.any(1), rel.int().argmax(1), m)  # the first relevant position, m if none
    n_id = min(ideal.shape[1], m)
    idcg_cum = torch.cumsum(gain[ideal[:, :n_id].long()] * discount[None, :n_id], 1)
    R = rel_rows[rows]
    fR = R.float().clamp(min=1.0)
    out = torch.zeros((nq, len(ks), 8), dtype=torch.float32, device=doc.device)
    hits, judged = [], []
    for ik, k in enumerate(ks):
        n = min(k, m)
        h, dcg, idcg = hits_cum[:, n - 1], dcg_cum[:, n - 1], idcg_cum[rows, min(k, n_id) - 1]
        hits.append(h), judged.append(judged_cum[:, n - 1])
        out[:, ik, 0] = torch.where(idcg > 0, dcg / idcg, 0.0)
        out[:, ik, 1] = torch.where(R > 0, ap_cum[:, n - 1] / fR, 0.0)
        out[:, ik, 2] = torch.where(R > 0, h.float() / fR, 0.0)
        out[:, ik, 3] = h.float() / float(k)
        out[:, ik, 4] = torch.where(first < n, 1.0 / (first + 1).float(), 0.0)
        out[:, ik, 5] = (h > 0).float()
        out[:, ik, 6], out[:, ik, 7] = dcg, idcg
    return out, torch.stack(hits, 1).int(), torch.stack(judged, 1).int(), R.int(), out.double().mean(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="1 024 lists only")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    print(f"# lists of docs of a {N_DOCS}-doc corpus, a third of the positions judged; cutoffs {KS}; linear gains over {N_GAIN} grades; per-query metrics and "
          f"means; median (min .. max) ms of {a.iters} repetitions after {a.warmup} warm-up, hipEvents on the current stream; {torch.cuda.get_device_name(0)}",
          flush=True)
    n_rows = 1024
    for row_len in (16, 256, 4096):
        doc2, grade2, ideal2 = make_rows(gen, n_rows, row_len, dev)
        j_ptr = np.arange(n_rows + 1, dtype=np.int64) * row_len
        j = ev.Judgments(j_ptr, doc2.cpu().numpy().reshape(-1), grade2.cpu().numpy().reshape(-1), ideal2.cpu().numpy().reshape(-1), device=dev)
        key_j = (torch.arange(n_rows, device=dev)[:, None] * STRIDE + doc2.long()).reshape(-1)
        grade_flat = grade2.reshape(-1).long()
        rel_rows = (grade2.clamp(0, N_GAIN - 1) >= REL_LEVEL).sum(1)
        for nq in ((1024,) if a.small else (1024, 65536)):
            q_rows = (torch.arange(nq, device=dev) % n_rows).int()
            for m in (128, 1024, 2048):
                ks = {128: [1, 10, 100, 129], 1024: [10, 100, 1000, 1025]}.get(m, list(KS))  # 4 cutoffs, one above a short list
                cand = torch.randint(0, N_DOCS, (nq, m), generator=gen, device=dev, dtype=torch.int64)
                own = torch.gather(doc2.long()[q_rows.long()], 1, torch.randint(0, row_len, (nq, m), generator=gen, device=dev))
                doc = torch.where(torch.rand((nq, m), generator=gen, device=dev) < 1 / 3, own, cand).int().contiguous()
                del cand, own
                gain, discount = j.tables("linear", m, N_GAIN)
                kernel = lambda: j.evaluate_device(doc, None, ks, q_rows, n_gain=N_GAIN)
                route = lambda: torch_eval(key_j, grade_flat, ideal2, rel_rows, gain, discount, doc, q_rows, ks)
                t, tt = timed(kernel, a.iters, a.warmup), timed(route, a.iters, a.warmup)
                got, exp = kernel(), route()
                torch.cuda.synchronize()
                assert torch.equal(got.hits, exp[1]) and torch.equal(got.judged, exp[2]) and torch.equal(got.rel, exp[3]), "the torch route and the kernel disagree"
                assert int(got.n[0]) == nq
                diff = float((got.out - exp[0]).abs().max()), float((got.mean - exp[4]).abs().max())
                name = f"{nq:5d} lists, m = {m:4d}, rows of {row_len:4d}, {len(ks)} cutoffs"
                line(f"{name}: srx_eval_lists", t)
                line(f"{name}: torch ops on the same GPU", tt,
                     f"   kernel / torch time {t[0] / tt[0]:.2f} (spreads: kernel {t[2] - t[1]:.3f} ms, torch {tt[2] - tt[1]:.3f} ms; difference "
                     f"{tt[0] - t[0]:.3f} ms); largest |difference| per query {diff[0]:.2e}, of a mean {diff[1]:.2e}; mean hits@{ks[-1]} "
                     f"{float(got.hits[:, -1].float().mean()):.1f}")
                del doc
        del j, key_j, grade_flat, doc2, grade2, ideal2


if __name__ == "__main__":
    main()
