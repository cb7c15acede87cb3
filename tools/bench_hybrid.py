"""Dev bench of hybrid retrieval: what the fusion kernel costs next to the two searches it follows, and next to fusing
on the host.  One process, one stream, device events around each step, warmed up.

  python tools/bench_hybrid.py [n_docs] [dim] [nq] [top_k] [iters]

Per shape (candidates = top_k, then candidates = 1000): sparse search ms (a C2-like BM25 index: uniform corpus, 50 terms
per doc, 8-term queries), dense INT8 search ms, srx_fuse_topk ms, the host-side alternative (both result sets copied
to the host and fused there by the vectorised NumPy routine below -- what a caller had to do before this entry point;
it is also checked against the kernel's rows, bit for bit), and the algorithmic bytes of the fusion over its time."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import sparse_rx
from sparse_rx import synth

n_docs = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
nq = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
top_k = int(sys.argv[4]) if len(sys.argv) > 4 else 100
iters = int(sys.argv[5]) if len(sys.argv) > 5 else 100
host_iters = max(5, iters // 5)
VOCAB, NNZ_PER_DOC, TERMS, SEED = 50_000, 50, 8, 20252
dev = torch.device("cuda:0")


def host_fuse(a, b, k, mode, wa, wb, rrf_c):
    """Vectorised NumPy fusion of two host result sets (same contract as the kernel): contributions, one sort by doc per
    query to find the docs both lists hold, one lexsort by (score desc, doc asc)."""
    def contributions(d, s, c, w):
        kx = d.shape[1]
        r = np.arange(kx, dtype=np.int32)[None, :]
        used = (r < np.clip(c, 0, kx)[:, None]) & (d >= 0) & (s > 0)
        if mode == "weighted":
            used &= used[:, :1]
            with np.errstate(all="ignore"):
                v = np.float32(w) * (s / np.where(s[:, :1] > 0, s[:, :1], np.float32(1)))
        else:
            v = np.broadcast_to(np.float32(w) / (np.float32(rrf_c) + (r + 1).astype(np.float32)), d.shape)
        return np.where(used, v, np.float32(0)).astype(np.float32)

    c = np.concatenate([contributions(*a, wa), contributions(*b, wb)], axis=1)
    doc = np.where(c > 0, np.concatenate([a[0], b[0]], axis=1), np.iinfo(np.int32).max)
    order = np.argsort(doc, axis=1, kind="stable")
    doc, c = np.take_along_axis(doc, order, 1), np.take_along_axis(c, order, 1)
    same = (doc[:, 1:] == doc[:, :-1]) & (c[:, 1:] > 0)  # a doc is at most once in each list: pairs only
    c[:, :-1] += np.where(same, c[:, 1:], np.float32(0))
    c[:, 1:][same] = 0
    rank = np.lexsort((doc, -c), axis=1)[:, :k]
    doc, c = np.take_along_axis(doc, rank, 1), np.take_along_axis(c, rank, 1)
    if doc.shape[1] < k:
        doc = np.pad(doc, ((0, 0), (0, k - doc.shape[1])), constant_values=-1)
        c = np.pad(c, ((0, 0), (0, k - c.shape[1])))
    keep = c > 0
    return np.where(keep, doc, -1).astype(np.int32), np.where(keep, c, 0).astype(np.float32), keep.sum(axis=1).astype(np.int32)


def stats(x):
    x = np.sort(np.asarray(x))
    return f"median {np.median(x):.4f} ms (p10 {x[len(x) // 10]:.4f}, p90 {x[(9 * len(x)) // 10]:.4f}, n={len(x)})"


# ---- the two indexes over the same rows ---------------------------------------------------------------------------------
t0 = time.perf_counter()
rows, cols, tf, dl = synth.uniform_chunk_torch(0, n_docs, VOCAB, NNZ_PER_DOC, SEED, dev)
df = torch.bincount(cols, minlength=VOCAB).cpu().numpy()
idf = torch.as_tensor(np.log((n_docs - df + 0.5) / (df + 0.5)).astype(np.float32), device=dev)
ix = sparse_rx.DeviceIndex.from_coo(rows, cols, tf, idf, n_docs, doc_lengths=dl, avgdl=float(dl.mean().item()), device=dev,
                                    keep_canonical=False)
del rows, cols, tf
q_ptr, q_term, q_w = (torch.as_tensor(x, device=dev) for x in synth.queries_np(nq, VOCAB, TERMS, SEED + 1))
g = torch.Generator(device=dev); g.manual_seed(1)
c8 = torch.randint(-127, 128, (n_docs, dim), generator=g, device=dev, dtype=torch.int32).to(torch.int8)
dx = sparse_rx.DenseInt8Index(c8, torch.rand(n_docs, generator=g, device=dev) + 0.01)
del c8
q8 = torch.randint(-127, 128, (nq, dim), generator=g, device=dev, dtype=torch.int32).to(torch.int8)
qs = (torch.rand(nq, generator=g, device=dev) + 0.01) / 127
torch.cuda.synchronize()
print(f"hybrid bench on {torch.cuda.get_device_name(0)}: {n_docs} docs (sparse: vocab {VOCAB}, {NNZ_PER_DOC} terms/doc, {TERMS}-term queries; "
      f"dense: int8 x {dim}), {nq} queries, top_k {top_k}, {iters} timed iterations after 10 warm-up; built in {time.perf_counter() - t0:.1f} s")

for cand in (top_k, 1000):
    for mode in ("weighted", "rrf"):
        w = (0.3, 0.7)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(iters)]
        for it in range(-10, iters):
            e = ev[max(it, 0)]
            e[0].record()
            a = ix.search_device(q_ptr, q_term, q_w, cand)
            e[1].record()
            b = dx.search_device(q8, qs, cand)
            e[2].record()
            f = sparse_rx.fuse_topk_device(a, b, top_k, mode=mode, weights=w)
            e[3].record()
        torch.cuda.synchronize()
        ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(3)] for e in ev])
        # the host-side alternative: six copies + NumPy
        host = []
        for _ in range(host_iters):
            t1 = time.perf_counter()
            ha, hb = tuple(x.cpu().numpy() for x in a), tuple(x.cpu().numpy() for x in b)
            t2 = time.perf_counter()
            hf = host_fuse(ha, hb, top_k, mode, w[0], w[1], 60.0)
            host.append(((t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3))
        host = np.array(host)
        gf = tuple(x.cpu().numpy() for x in f)
        same = np.array_equal(gf[2], hf[2]) and np.array_equal(gf[0], hf[0]) and np.array_equal(gf[1].view(np.uint32), hf[1].view(np.uint32))
        nbytes = nq * (2 * cand + top_k) * 8 + 3 * nq * 4
        fuse_ms = float(np.median(ms[:, 2]))
        print(f"[candidates {cand}, {mode}] form: {'wave' if 2 * cand <= 1024 and top_k <= 128 else 'block'}; "
              f"mean lists: sparse {float(a[2].float().mean()):.0f}, dense {float(b[2].float().mean()):.0f}, fused {float(f[2].float().mean()):.0f} rows")
        print(f"    sparse search  {stats(ms[:, 0])}")
        print(f"    dense search   {stats(ms[:, 1])}")
        print(f"    srx_fuse_topk  {stats(ms[:, 2])}; {nbytes / 1e6:.2f} MB algorithmic -> {nbytes / fuse_ms / 1e6:.1f} GB/s")
        print(f"    host route     copies {stats(host[:, 0])} + NumPy fusion {stats(host[:, 1])}; "
              f"total median {np.median(host.sum(axis=1)):.3f} ms = {np.median(host.sum(axis=1)) / fuse_ms:.0f} x the kernel; "
              f"rows {'equal bit for bit' if same else 'DIFFER'}")
        assert same, "host fusion and kernel disagree"
ix.close()
