"""What a term constraint costs: per corpus,

  1. the builder: ``srx_filter_from_terms`` for ``--rows`` rows of (1 must, 1 must-not) terms, once with the corpus' rarest terms
     and once with its most frequent ones, and the same rows over a density-0.5 base;
  2. the constrained search: one batch of ``--rows`` queries, query i under row i,
       a. with the term-built rows (the search alone, and builder + search: what a constrained API call pays on the device);
       b. with the equivalent rows given through ``DocFilter.from_masks`` (host masks packed and uploaded -- the route a caller
          had before; the masks are read back from the built rows, so building them on the host is NOT in the time);
       c. unfiltered, for scale,

each the median of ``--iters`` hipEvent-timed repetitions after ``--warmup``, same device tensors, same stream.  The host route
of 2b is measured on ``--host-rows`` rows and scaled (default: all rows, 32 at c3 size, where a mask is 10 MB of bools per row).

    python tools/bench_terms.py [--corpus uniform100k|zipf100k|c3] [--rows 1000] [--iters 20] [--warmup 5]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparse_rx  # noqa: E402
from sparse_rx import synth  # noqa: E402
from bench_filtered import build as build_uniform, timed  # noqa: E402


def build(corpus, dev):
    if corpus != "zipf100k":
        return build_uniform(corpus, dev)
    c = synth.zipf_corpus_np(100_000, 20_000, 40, seed=72, s=1.0)  # the zipf corpus of tests/test_search_plans.py: really hot terms
    _, idf, avgdl = synth.corpus_stats(c)
    ix = sparse_rx.DeviceIndex.from_csr(c.indptr, c.indices, c.data, idf, doc_lengths=c.doc_lengths, avgdl=avgdl, device=dev, tile_log2=10,
                                        unit_tiles=4, keep_canonical=False)
    return ix, 20_000, 8, 73


def term_df(ix):
    """Stored postings per term, padding included (<= 3 per unit and term): good enough to rank terms by frequency"""
    skip = ix.tile_skip.view(ix.vocab, ix.n_tiles + 1)
    return skip[:, -1].cpu().numpy().astype(np.int64)


def csr_pairs(terms, dev):
    ptr = torch.arange(len(terms) + 1, dtype=torch.int32, device=dev)
    return ptr, torch.as_tensor(np.asarray(terms, np.int32), device=dev)


def line(name, t, ref=None):
    rel = "" if ref is None else f"   {100.0 * (t[0] / ref - 1.0):+7.1f} % vs unfiltered"
    print(f"{name:66s} {t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){rel}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="uniform100k", choices=["uniform100k", "zipf100k", "c3"])
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=0, help="rows of the host route (0: all of them, 32 at c3 size)")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ix, V, terms, qseed = build(a.corpus, dev)
    if ix.post is not None:
        ix.drop_canonical()  # what the API mirrors keep resident: the builder reads the compact copy
    n = a.rows
    df = term_df(ix)
    order = np.argsort(df, kind="stable")
    order = order[df[order] > 0]
    rare, hot = order[:2 * n], order[::-1][:2 * n]
    unit_docs = ix.unit_tiles << ix.tile_log2
    print(f"# {a.corpus}: {ix.n_docs} docs, vocab {V}, units of {unit_docs} docs ({-(-ix.n_docs // unit_docs)} per row), {n} rows = "
          f"{n * sparse_rx.filter.filter_words(ix.n_docs) * 4 / 2 ** 20:.1f} MiB of filter; median (min .. max) ms of {a.iters} repetitions after "
          f"{a.warmup} warm-up, hipEvents on the current stream; {torch.cuda.get_device_name(0)}; kernel sources "
          f"{sparse_rx._capi.kernel_sources_sha256()[:16]}", flush=True)
    print(f"# postings per term: rare rows {int(df[rare].min())} .. {int(df[rare].max())}, hot rows {int(df[hot].min())} .. {int(df[hot].max())}", flush=True)
    out = torch.empty((n, sparse_rx.filter.filter_words(ix.n_docs)), dtype=torch.int32, device=dev)
    base = sparse_rx.DocFilter.from_masks(np.random.default_rng(5).random(ix.n_docs) < 0.5, device=dev, doc_base=ix.doc_base)
    built = {}
    for name, pick in (("rare", rare), ("hot", hot)):
        must, must_not = csr_pairs(pick[:n], dev), csr_pairs(pick[n:2 * n], dev)
        built[name] = (must, must_not)
        line(f"builder, {n} rows of 1 must + 1 must-not, {name} terms", timed(lambda: ix.term_filter_device(must, None, must_not, out=out), a.iters, a.warmup))
        line(f"builder, the same over a density-0.5 base row, {name} terms",
             timed(lambda: ix.term_filter_device(must, None, must_not, base=base, out=out), a.iters, a.warmup))
        line(f"builder, {n} rows of 1 must only, {name} terms", timed(lambda: ix.term_filter_device(must, out=out), a.iters, a.warmup))
    # ---- the constrained search: query i under row i
    q = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in synth.queries_np(n, V, terms, seed=qseed)]
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    res = ix.search_device(*q, a.k)
    plain = timed(lambda: ix.search_device(*q, a.k, out=res), a.iters, a.warmup)
    line(f"search, {n} queries x {terms} terms, k = {a.k}, unfiltered", plain)
    for name in ("rare", "hot"):
        must, must_not = built[name]
        flt = ix.term_filter_device(must, None, must_not, out=out)
        torch.cuda.synchronize()
        allowed = flt.count()
        print(f"# {name} rows allow {int(allowed.min())} .. {int(allowed.max())} docs", flush=True)
        line(f"search under the term-built rows ({name})", timed(lambda: ix.search_device(*q, a.k, out=res, filter=flt, q_filter=rows), a.iters, a.warmup), plain[0])

        def both():
            f = ix.term_filter_device(must, None, must_not, out=out)
            ix.search_device(*q, a.k, out=res, filter=f, q_filter=rows)
        line(f"builder + search ({name})", timed(both, a.iters, a.warmup), plain[0])
        # the host route: the same rows as bool masks, packed and uploaded by DocFilter.from_masks
        h = min(n, a.host_rows if a.host_rows > 0 else 32 if a.corpus == "c3" else n)
        bits = out[:h].cpu().numpy().view(np.uint32)
        masks = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, : ix.n_docs].astype(bool)
        t0 = time.perf_counter()
        host = sparse_rx.DocFilter.from_masks(masks, device=dev, doc_base=ix.doc_base)
        torch.cuda.synchronize()
        t_up = (time.perf_counter() - t0) * 1e3
        assert torch.equal(host.bits, out[:h])
        print(f"{'DocFilter.from_masks of ' + str(h) + ' equivalent rows (pack + upload, wall clock)':66s} {t_up:9.3f} ms  -> {t_up * n / h:.1f} ms for {n} rows", flush=True)
        if h == n:
            line(f"search under the from_masks rows ({name})", timed(lambda: ix.search_device(*q, a.k, out=res, filter=host, q_filter=rows), a.iters, a.warmup), plain[0])
        else:
            print(f"# search under from_masks rows: the same bits in the same layout as the term-built rows (checked on {h} rows), so the same search", flush=True)
        del host, masks
    ix.close()


if __name__ == "__main__":
    main()
