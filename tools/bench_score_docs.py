"""Dev bench of srx_score_docs: what scoring caller-given candidates costs next to the search of the same batch, and next
to the only route a caller had before this entry point.  One process, one stream, device events around each call, warmed up.

  python tools/bench_score_docs.py [--docs N] [--nq N] [--iters N] [--kernels-only]

Set-up: a C2-like BM25 index (uniform corpus, 50 terms per doc, vocabulary 50 000), 1 024 queries x 8 terms, in two resident
layouts -- "compact" (one copy of the postings: the 16-bit-id blocks, the product default) and "canonical" (units of
65 536 docs, for which no compact copy exists: the 32-bit-id blocks).  Per layout and m in {100, 1 000}, candidates once = the
batch's own search rows and once uniformly random docs:
  * srx_score_docs          median and p10-p90 over the timed iterations;
  * (a) srx_search          of the same batch at k = m on the same index;
  * (b) the host route      candidates copied to the host and looked up in the host CSR with vectorised NumPy (impacts,
                            idf, query weights and the ordered fp32 sum restated there) -- checked against the kernel's
                            rows bit for bit in every run.
--kernels-only runs the device calls alone (fewer iterations, no host route): the run to wrap in
``rocprofv3 --kernel-trace --stats`` for the kernels' own durations."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sparse_rx
from sparse_rx import synth

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--nq", type=int, default=1024)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--kernels-only", action="store_true")
args = ap.parse_args()
n_docs, nq, iters = args.docs, args.nq, (20 if args.kernels_only else args.iters)
VOCAB, NNZ_PER_DOC, TERMS, SEED, K1, B = 50_000, 50, 8, 20252, 1.2, 0.75
dev = torch.device("cuda:0")


def stats(x):
    x = np.sort(np.asarray(x))
    return f"median {np.median(x):.4f} ms (p10 {x[len(x) // 10]:.4f}, p90 {x[(9 * len(x)) // 10]:.4f}, n={len(x)})"


def host_route(host, q, cand, count):
    """Scores of a candidate block from the doc-major host CSR: per query term position i, one searchsorted of
    (doc, term) in the CSR's globally ascending (row * vocab + col) keys, the BM25 impact in the reference's fp32 operation
    order, (impact * idf) * qw, added in term order."""
    keys, tf, dl, idf, avgdl = host
    f = np.float32
    q_ptr, q_term, q_w = q
    m = cand.shape[1]
    live = (cand >= 0) & (cand < n_docs) & (np.arange(m)[None, :] < np.maximum(count, 0)[:, None])
    doc = np.where(live, cand, 0).astype(np.int64)
    norm = f(K1) * (f(1.0 - B) + (f(B) * dl[doc]) / f(avgdl))
    s = np.zeros(cand.shape, f)
    nt = np.diff(q_ptr)
    for i in range(int(nt.max())):
        has = nt > i
        at = np.minimum(q_ptr[:-1] + i, len(q_term) - 1)
        t, w = q_term[at].astype(np.int64), q_w[at]
        key = doc * VOCAB + t[:, None]
        pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
        hit = (keys[pos] == key) & live & has[:, None]
        v = tf[pos]
        imp = (v * f(K1 + 1.0)) / (v + norm)
        s = np.where(hit, s + (imp * idf[t][:, None]) * w[:, None], s).astype(f)
    return s


t0 = time.perf_counter()
rows, cols, tf, dl = synth.uniform_chunk_torch(0, n_docs, VOCAB, NNZ_PER_DOC, SEED, dev)
df = torch.bincount(cols, minlength=VOCAB).cpu().numpy()
idf_np = np.log((n_docs - df + 0.5) / (df + 0.5)).astype(np.float32)
avgdl = float(dl.mean().item())
q = synth.queries_np(nq, VOCAB, TERMS, SEED + 1)
dq = [torch.as_tensor(x, device=dev) for x in q]
host = None
if not args.kernels_only:
    host = ((rows.to(torch.int64) * VOCAB + cols.to(torch.int64)).cpu().numpy(), tf.cpu().numpy(), dl.cpu().numpy(), idf_np, avgdl)
    assert np.all(np.diff(host[0]) > 0)
print(f"score_docs bench on {torch.cuda.get_device_name(0)}: {n_docs} docs (vocab {VOCAB}, {NNZ_PER_DOC} terms/doc), {nq} queries x {TERMS} terms, "
      f"{iters} timed iterations after 10 warm-up; kernel sources {sparse_rx._capi.kernel_sources_sha256()[:16]}", flush=True)

for layout, kw in (("compact", dict(keep_canonical=False)), ("canonical", dict(tile_log2=14, unit_tiles=4))):
    ix = sparse_rx.DeviceIndex.from_coo(rows, cols, tf, torch.as_tensor(idf_np, device=dev), n_docs, doc_lengths=dl, avgdl=avgdl, device=dev, **kw)
    assert (ix.post16 is None) == (layout == "canonical")
    print(f"[{layout}] tile_log2 {ix.tile_log2}, unit_tiles {ix.unit_tiles}, resident {ix.device_bytes() / 2 ** 20:.0f} MiB, built {time.perf_counter() - t0:.1f} s "
          f"after start", flush=True)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    for m in (100, 1000):
        own = ix.search_device(*dq, m)
        rnd = (torch.randint(0, n_docs, (nq, m), generator=g, device=dev, dtype=torch.int32), torch.full((nq,), m, dtype=torch.int32, device=dev))
        out = torch.empty((nq, m), dtype=torch.float32, device=dev)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(iters)]
        for it in range(-10, iters):
            e = ev[max(it, 0)]
            e[0].record()
            srch = ix.search_device(*dq, m)
            e[1].record()
            ix.score_docs_device(*dq, own[0], own[2], out=out)
            e[2].record()
            ix.score_docs_device(*dq, rnd[0], rnd[1], out=out)
            e[3].record()
        torch.cuda.synchronize()
        ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(3)] for e in ev])
        same_rows = bool(torch.equal(ix.score_docs_device(*dq, own[0], own[2]).view(torch.int32), own[1].view(torch.int32)))
        print(f"  [m = {m}] pairs {nq * m}; mean rows per query {float(own[2].float().mean()):.0f}")
        print(f"    (a) srx_search k = m          {stats(ms[:, 0])}")
        print(f"    srx_score_docs, own rows      {stats(ms[:, 1])}; equal to the rows' own scores bit for bit: {same_rows}")
        print(f"    srx_score_docs, random docs   {stats(ms[:, 2])}")
        assert same_rows
        if host is not None:
            for name, (cd, cc) in (("own rows", (own[0], own[2])), ("random docs", rnd)):
                got = ix.score_docs_device(*dq, cd, cc).cpu().numpy()
                t1 = time.perf_counter()
                hc, hn = cd.cpu().numpy(), cc.cpu().numpy()
                t2 = time.perf_counter()
                hs = host_route(host, q, hc, hn)
                t3 = time.perf_counter()
                same = np.array_equal(hs.view(np.uint32), got.view(np.uint32))
                print(f"    (b) host route, {name:<12}  copies {(t2 - t1) * 1e3:.2f} ms + NumPy lookup {(t3 - t2) * 1e3:.1f} ms; rows "
                      f"{'equal bit for bit' if same else 'DIFFER'}", flush=True)
                assert same, "host route and kernel disagree"
    ix.close()
