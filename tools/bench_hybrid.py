"""Dev bench of hybrid retrieval: what the fusion kernel costs next to the two searches it follows, and next to fusing
on the host.  One process, one stream, device events around each step, warmed up.

  python tools/bench_hybrid.py [n_docs] [dim] [nq] [top_k] [iters]

Per shape (candidates = top_k, then candidates = 1000): sparse search ms (a C2-like BM25 index: uniform corpus, 50 terms
per doc, 8-term queries), dense INT8 search ms, srx_fuse_topk ms, the host-side alternative (both result sets copied
to the host and fused there by the vectorised NumPy routine below -- what a caller had to do before this entry point;
it is also checked against the kernel's rows, bit for bit), and the algorithmic bytes of the fusion over its time.

Then the rescore leg (weighted fusion) at the same two depths: device events around each of its five steps
-- sparse search, dense search, srx_score_docs over the dense rows, srx_dense_score_docs_i8 over the sparse rows,
srx_fuse_topk_scored -- and the route a caller had before the dense scorer and the scored fusion existed: the rows of
the two searches and of srx_score_docs copied to the host, the dense completion (a gather of the INT8 rows and an exact
dot product) and the fusion done in NumPy; its rows are checked against the kernels' bit for bit in every run.  Last,
each dense score kernel (i8 packed and row-major, f32, u8) next to its own search at k = m.  ``--no-plain`` skips the
plain legs, ``--no-kernels`` the last part."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import sparse_rx
from sparse_rx import synth

flags = {a for a in sys.argv[1:] if a.startswith("--")}
sys.argv = [a for a in sys.argv if a not in flags]
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


def host_fuse_scored(a, a_other, b, b_other, k, wa, wb):
    """Vectorised NumPy form of srx_fuse_topk_scored (include/sparse_rx_rescore.h): every used entry fuses its two scores,
    an entry of B whose doc is a used entry of A is dropped (one sort by (doc, list) per query), one lexsort by
    (score desc, doc asc)."""
    def used_head(d, s, c):
        kx = d.shape[1]
        used = (np.arange(kx, dtype=np.int32)[None, :] < np.clip(c, 0, kx)[:, None]) & (d >= 0) & (s > 0)
        return used, np.where(used[:, :1], s[:, :1], np.float32(0))  # head 0 = no normaliser

    ua, ma = used_head(*a)
    ub, mb = used_head(*b)

    def contribution(s, w, m):
        with np.errstate(all="ignore"):
            v = np.float32(w) * (s / np.where(m > 0, m, np.float32(1)))
        return np.where((m > 0) & (s > 0), v, np.float32(0)).astype(np.float32)

    fa = np.where(ua, contribution(a[1], wa, ma) + contribution(a_other, wb, mb), np.float32(0))
    fb = np.where(ub, contribution(b_other, wa, ma) + contribution(b[1], wb, mb), np.float32(0))
    big = np.iinfo(np.int32).max
    doc = np.concatenate([np.where(ua, a[0], big), np.where(ub, b[0], big)], axis=1)
    c = np.concatenate([fa, fb], axis=1).astype(np.float32)
    order = np.argsort(doc, axis=1, kind="stable")  # stable: of two equal docs list A's entry comes first
    doc, c = np.take_along_axis(doc, order, 1), np.take_along_axis(c, order, 1)
    c[:, 1:][(doc[:, 1:] == doc[:, :-1]) & (doc[:, 1:] != big)] = 0
    c = np.where(c > 0, c, np.float32(0))  # NaN and unused entries rank nowhere
    rank = np.lexsort((doc, -c), axis=1)[:, :k]
    doc, c = np.take_along_axis(doc, rank, 1), np.take_along_axis(c, rank, 1)
    if doc.shape[1] < k:
        doc = np.pad(doc, ((0, 0), (0, k - doc.shape[1])), constant_values=-1)
        c = np.pad(c, ((0, 0), (0, k - c.shape[1])))
    keep = c > 0
    return np.where(keep, doc, -1).astype(np.int32), np.where(keep, c, 0).astype(np.float32), keep.sum(axis=1).astype(np.int32)


def host_dense_i8(c8_host, cs_host, q8_host, qs_host, doc, count):
    """The dense completion on the host: exact integer dots of the gathered INT8 rows (fp32 accumulation is exact: every
    partial sum is an integer below 2^24 for rows of <= 1 040 bytes), then the engine's fp64 scaling"""
    out = np.zeros(doc.shape, np.float32)
    live = (np.arange(doc.shape[1])[None, :] < np.clip(count, 0, None)[:, None]) & (doc >= 0)
    qf = q8_host.astype(np.float32)
    step = max(1, (256 << 20) // (doc.shape[1] * c8_host.shape[1] * 4))
    for lo in range(0, len(doc), step):
        d = np.where(live[lo: lo + step], doc[lo: lo + step], 0)
        acc = np.einsum("qmd,qd->qm", c8_host[d].astype(np.float32), qf[lo: lo + step])
        sc = ((acc.astype(np.float64) * qs_host[lo: lo + step, None].astype(np.float64)) * cs_host[d].astype(np.float64)).astype(np.float32)
        out[lo: lo + step] = np.where(live[lo: lo + step], sc, np.float32(0))
    return out


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
c8_host = c8.cpu().numpy()  # the host route of the rescore leg completes the sparse list from this copy
del c8
q8 = torch.randint(-127, 128, (nq, dim), generator=g, device=dev, dtype=torch.int32).to(torch.int8)
qs = (torch.rand(nq, generator=g, device=dev) + 0.01) / 127
torch.cuda.synchronize()
print(f"hybrid bench on {torch.cuda.get_device_name(0)}: {n_docs} docs (sparse: vocab {VOCAB}, {NNZ_PER_DOC} terms/doc, {TERMS}-term queries; "
      f"dense: int8 x {dim}), {nq} queries, top_k {top_k}, {iters} timed iterations after 10 warm-up; built in {time.perf_counter() - t0:.1f} s")

for cand in (top_k, 1000):
    for mode in ("weighted", "rrf") if "--no-plain" not in flags else ():
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

# ---- the rescore leg: five steps on the device, and the host route to the same rows ----------------------------------------
cs_host, q8_host, qs_host = dx.scales.cpu().numpy(), q8.cpu().numpy(), qs.cpu().numpy()
STEPS = ("sparse search", "dense search", "srx_score_docs (dense rows)", "srx_dense_score_docs_i8 (sparse rows)", "srx_fuse_topk_scored")
for cand in (top_k, 1000):
    w = (0.3, 0.7)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(iters)]
    for it in range(-10, iters):
        e = ev[max(it, 0)]
        e[0].record()
        a = ix.search_device(q_ptr, q_term, q_w, cand)
        e[1].record()
        b = dx.search_device(q8, qs, cand)
        e[2].record()
        b_other = ix.score_docs_device(q_ptr, q_term, q_w, b[0], b[2])
        e[3].record()
        a_other = dx.score_docs_device(q8, qs, a[0], a[2])
        e[4].record()
        f = sparse_rx.fuse_scored_device(a, a_other, b, b_other, top_k, w)
        e[5].record()
    torch.cuda.synchronize()
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(5)] for e in ev])
    total = np.array([e[0].elapsed_time(e[5]) for e in ev])
    host = []
    for _ in range(max(3, host_iters // 5)):
        t1 = time.perf_counter()
        ha, hb, hbo = tuple(x.cpu().numpy() for x in a), tuple(x.cpu().numpy() for x in b), b_other.cpu().numpy()
        t2 = time.perf_counter()
        hao = host_dense_i8(c8_host, cs_host, q8_host, qs_host, ha[0], ha[2])
        t3 = time.perf_counter()
        hf = host_fuse_scored(ha, hao, hb, hbo, top_k, w[0], w[1])
        host.append(((t2 - t1) * 1e3, (t3 - t2) * 1e3, (time.perf_counter() - t3) * 1e3))
    host = np.array(host)
    gf = tuple(x.cpu().numpy() for x in f)
    same = (np.array_equal(hao.view(np.uint32), a_other.cpu().numpy().view(np.uint32)) and np.array_equal(gf[2], hf[2])
            and np.array_equal(gf[0], hf[0]) and np.array_equal(gf[1].view(np.uint32), hf[1].view(np.uint32)))
    print(f"[rescore, candidates {cand}] form: {'wave' if 2 * cand <= 1024 and top_k <= 128 else 'block'}; mean lists: sparse "
          f"{float(a[2].float().mean()):.0f}, dense {float(b[2].float().mean()):.0f}, fused {float(f[2].float().mean()):.0f} rows")
    for i, name in enumerate(STEPS):
        print(f"    {name:38s} {stats(ms[:, i])}")
    after = float(np.median(ms[:, 2:].sum(axis=1)))  # what follows the two searches on the device ...
    host_after = float(np.median(host.sum(axis=1)))  # ... and what followed them (and srx_score_docs) on the host route
    print(f"    five steps, first event to last        {stats(total)}; steps 3-5, after the two searches: median {after:.4f} ms")
    print(f"    host route after the two searches and srx_score_docs: copies {stats(host[:, 0])} + NumPy dense completion {stats(host[:, 1])} + "
          f"NumPy fusion {stats(host[:, 2])}; total median {host_after:.1f} ms, against {float(np.median(ms[:, 3:].sum(axis=1))):.4f} ms for the two "
          f"steps it replaces (steps 4-5); rows {'equal bit for bit' if same else 'DIFFER'}")
    assert same, "host route and kernels disagree"
ix.close()

# ---- each dense score kernel next to its own search at k = m ---------------------------------------------------------------
def kernel_vs_search(name, index, qargs, m, n_it):
    d, _, n = index.search_device(*qargs, m)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n_it)]
    for it in range(-3, n_it):
        e = ev[max(it, 0)]
        e[0].record()
        index.search_device(*qargs, m)
        e[1].record()
        index.score_docs_device(*qargs, d, n)
        e[2].record()
    torch.cuda.synchronize()
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(2)] for e in ev])
    row_bytes = index.dim_pad * (4 if isinstance(index, sparse_rx.DenseF32Index) else 1)
    gbs = float(n.sum()) * row_bytes / np.median(ms[:, 1]) / 1e6
    print(f"[{name}, m = k = {m}] search {stats(ms[:, 0])}; score kernel {stats(ms[:, 1])} = 1/{np.median(ms[:, 0]) / np.median(ms[:, 1]):.0f} of "
          f"the search; {gbs:.0f} GB/s of gathered rows")


if "--no-kernels" not in flags:
    for m in (top_k, 1000):
        kernel_vs_search("i8 packed", dx, (q8, qs), m, iters)
    cs_dev = dx.scales
    del dx
    rm = sparse_rx.DenseInt8Index(torch.as_tensor(c8_host), cs_dev, packed=False)
    for m in (top_k, 1000):
        kernel_vs_search("i8 row-major", rm, (q8, qs), m, iters)
    del rm
    qf = torch.randn((nq, dim), generator=g, device=dev)
    u8 = sparse_rx.DenseUint8Index((c8_host.view(np.uint8)), np.stack([np.full(n_docs, 0.01, np.float32), np.full(n_docs, -1.27, np.float32)], axis=1).reshape(-1))
    for m in (top_k, 1000):
        kernel_vs_search("u8", u8, (qf,), m, max(3, iters // 20))  # the f32 / u8 searches stream the corpus once per 4 queries
    del u8
    fx = sparse_rx.DenseF32Index(torch.randn((n_docs, dim), generator=g, device=dev))
    for m in (top_k, 1000):
        kernel_vs_search("f32", fx, (qf,), m, max(3, iters // 20))
