"""What a field predicate costs: per corpus size,

  1. the builder: ``srx_filter_from_fields`` for ``--rows`` rows of (a range on an int64 column, an ``in`` of 4 on a category
     column, a ``must_not`` ``any_of`` on a set column), the same rows over a density-0.5 base, and the same rows with the range
     clause alone;
  2. two baselines for the same rows, measured in the same session:
       a. the host route of today: NumPy masks, then ``DocFilter.from_masks`` (pack + upload), wall clock, on ``--host-rows`` rows
          and scaled (default: all rows, 32 at 10 M docs, where a mask is 10 MB of bools per row);
       b. the same predicate written in torch ops on the same GPU, the boolean expression packed to words, ``--torch-chunk`` rows
          at a time (a [rows, n_docs] intermediate is 10 GB at 1 000 rows x 10 M docs);
     the tool asserts that all three produce equal bits;
  3. the filtered search under these rows and under the equivalent ``from_masks`` rows (the same bits, so the same search),

each the median of ``--iters`` hipEvent-timed repetitions after ``--warmup``, same device tensors, same stream.

    python tools/bench_fields.py [--corpus uniform100k|c3] [--rows 1000] [--iters 20] [--warmup 5] [--no-search]
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
from sparse_rx.fields import WhereResolver  # noqa: E402
from sparse_rx.filter import filter_words  # noqa: E402
from bench_filtered import build, timed  # noqa: E402

N_DOCS = {"uniform100k": 100_000, "c3": 10_000_000}
SOURCES = [f"src{i:02d}" for i in range(16)]
LABELS = [f"tag{i:02d}" for i in range(12)]
CHUNK_DOCS, CHUNKS_PER_ROW, MAX_BATCH_ROWS = 2048, 8, 16  # csrc/fields.hip: docs per workgroup; rows per batch = chunks // 8 in [1, 16]


def line(name, t, note=""):
    print(f"{name:72s} {t[0]:9.3f} ms  ({t[1]:.3f} .. {t[2]:.3f}){note}", flush=True)


def make_fields(n, seed):
    rng = np.random.default_rng(seed)
    views = rng.integers(0, 1 << 40, n, dtype=np.int64)
    src = rng.integers(0, len(SOURCES), n).astype(np.int32)
    tags = rng.integers(0, 1 << len(LABELS), n, dtype=np.int64)
    return views, src, tags


def make_rows(n_rows, seed):
    """Per row: (lo, hi) of the range, 4 category codes, the label mask of the must-not"""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 1 << 39, n_rows, dtype=np.int64)
    hi = lo + rng.integers(1 << 38, 1 << 39, n_rows, dtype=np.int64)
    codes = np.stack([rng.choice(len(SOURCES), 4, replace=False) for _ in range(n_rows)]).astype(np.int64)
    labels = np.stack([rng.choice(len(LABELS), 2, replace=False) for _ in range(n_rows)])
    return lo, hi, codes, labels


def where_of(lo, hi, codes, labels, range_only):
    groups = []
    for r in range(len(lo)):
        g = {"must": [{"field": "views", "gte": int(lo[r]), "lte": int(hi[r])}]}
        if not range_only:
            g["must"].append({"field": "src", "in": [SOURCES[c] for c in codes[r]]})
            g["must_not"] = [{"field": "tags", "any_of": [LABELS[b] for b in labels[r]]}]
        groups.append(g)
    return groups


def device_call(table, groups, dev):
    """The device tensors of one builder call (resolved once, on the host), as filter_device takes them"""
    res = WhereResolver(table.columns)
    for g in groups:
        res.add(g)
    rec, values, lists = res.arrays()
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    return dict(clauses=up(rec), values=up(values) if len(values) else None, all=(up(lists[0][0]), up(lists[0][1])),
                none=(up(lists[2][0]), up(lists[2][1])), columns=res.names), len(res.clauses)


def torch_rows(views, src, tags, lo, hi, codes, mask, range_only, out, chunk):
    """The same predicate in torch ops, packed to filter words: `chunk` rows at a time"""
    n, words = views.numel(), out.shape[1]
    weights = (1 << torch.arange(8, device=views.device, dtype=torch.int32)).to(torch.uint8)
    for r0 in range(0, lo.numel(), chunk):
        r1 = min(r0 + chunk, lo.numel())
        ok = (views[None, :] >= lo[r0:r1, None]) & (views[None, :] <= hi[r0:r1, None])
        if not range_only:
            member = src[None, :] == codes[r0:r1, 0, None]
            for j in range(1, 4):
                member |= src[None, :] == codes[r0:r1, j, None]
            ok &= member
            ok &= (tags[None, :] & mask[r0:r1, None]) == 0
        padded = torch.zeros((r1 - r0, words * 32), dtype=torch.bool, device=views.device)
        padded[:, :n] = ok
        packed = (padded.view(r1 - r0, words * 4, 8).to(torch.uint8) * weights).sum(dim=2, dtype=torch.uint8)
        out[r0:r1] = packed.view(torch.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="uniform100k", choices=list(N_DOCS))
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=0, help="rows of the host route (0: all of them, 32 at c3 size)")
    ap.add_argument("--torch-chunk", type=int, default=0, help="rows per torch expression (0: 64, 8 at c3 size)")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-search", action="store_true", help="skip part 3 (it builds the sparse index of the corpus)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, n_rows = N_DOCS[a.corpus], a.rows
    words = filter_words(n)
    views, src, tags = make_fields(n, 7)
    # the category and the set column as their codes / bits with the dictionaries: what from_columns makes of strings, without 10 M of them
    table = sparse_rx.FieldTable.from_columns({"views": views, "src": sparse_rx.fields.HostColumn("category", src, None, SOURCES),
                                               "tags": sparse_rx.fields.HostColumn("set", tags, None, LABELS)}, device=dev)
    lo, hi, codes, labels = make_rows(n_rows, 8)
    n_chunks = -(-n // CHUNK_DOCS)
    batch = min(MAX_BATCH_ROWS, max(1, n_chunks // CHUNKS_PER_ROW))
    n_batches = -(-n_rows // batch)
    print(f"# {a.corpus}: {n} docs, {n_rows} rows = {n_rows * words * 4 / 2 ** 20:.1f} MiB of filter; columns {table.device_bytes() / 2 ** 20:.1f} MiB resident; "
          f"{n_chunks} chunks of {CHUNK_DOCS} docs, {n_batches} row batches of {batch}; median (min .. max) ms of {a.iters} repetitions after {a.warmup} warm-up, "
          f"hipEvents on the current stream; {torch.cuda.get_device_name(0)}", flush=True)
    out = torch.empty((n_rows, words), dtype=torch.int32, device=dev)
    base = sparse_rx.DocFilter.from_masks(np.random.default_rng(5).random(n) < 0.5, device=dev)
    d_views, d_src, d_tags = (torch.as_tensor(x, device=dev) for x in (views, src, tags))
    d_lo, d_hi, d_codes = (torch.as_tensor(x, device=dev) for x in (lo, hi, codes))
    d_codes32 = d_codes.to(torch.int32)
    mask = np.asarray([sum(1 << int(b) for b in row) for row in labels], dtype=np.int64)
    d_mask = torch.as_tensor(mask, device=dev)
    t_out = torch.empty_like(out)
    chunk = a.torch_chunk or (8 if n > 1_000_000 else 64)
    results = {}
    for range_only in (False, True):
        what = "range only" if range_only else "range + in of 4 + must_not any_of"
        call, n_clauses = device_call(table, where_of(lo, hi, codes, labels, range_only), dev)
        t = timed(lambda: table.filter_device(**call, out=out), a.iters, a.warmup)
        col_bytes = n * (8 if range_only else 8 + 4 + 8)  # from HBM once: the batches of a chunk run together and share it in L2
        moved = n_rows * words * 4 + col_bytes
        line(f"builder, {n_rows} rows, {what} ({n_clauses} clause records)", t,
             f"   {moved / t[0] / 1e9:.3f} TB/s of {moved / 2 ** 20:.0f} MiB (rows written + columns read once); the term builder's fold: 2.0 TB/s, roofline 8 TB/s")
        results[range_only] = t
        if not range_only:
            line("builder, the same over a density-0.5 base row", timed(lambda: table.filter_device(**call, base=base, out=out), a.iters, a.warmup))
        table.filter_device(**call, out=out)
        tt = timed(lambda: torch_rows(d_views, d_src, d_tags, d_lo, d_hi, d_codes32, d_mask, range_only, t_out, chunk), a.iters, a.warmup)
        line(f"torch ops on the same GPU, {chunk} rows per expression, packed to words ({what})", tt, f"   builder is {tt[0] / t[0]:.1f}x faster (spreads: builder "
             f"{t[2] - t[1]:.3f} ms, torch {tt[2] - tt[1]:.3f} ms)")
        torch.cuda.synchronize()
        assert torch.equal(t_out, out), "the torch restatement and the builder disagree"
        # the host route: NumPy masks, then pack + upload
        h = min(n_rows, a.host_rows if a.host_rows > 0 else 32 if n > 1_000_000 else n_rows)
        t0 = time.perf_counter()
        m = (views[None, :] >= lo[:h, None]) & (views[None, :] <= hi[:h, None])
        if not range_only:
            m &= (src[None, :] == codes[:h, 0, None]) | (src[None, :] == codes[:h, 1, None]) | (src[None, :] == codes[:h, 2, None]) | (src[None, :] == codes[:h, 3, None])
            m &= (tags[None, :] & mask[:h, None]) == 0
        t_mask = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host = sparse_rx.DocFilter.from_masks(m, device=dev)
        torch.cuda.synchronize()
        t_up = (time.perf_counter() - t0) * 1e3
        assert torch.equal(host.bits, out[:h]), "the host route and the builder disagree"
        print(f"{'host route on ' + str(h) + ' rows: NumPy masks ' + format(t_mask, '.1f') + ' ms + DocFilter.from_masks ' + format(t_up, '.1f') + ' ms (wall clock)':72s} "
              f"-> {(t_mask + t_up) * n_rows / h:.1f} ms for {n_rows} rows ({t_up * n_rows / h:.1f} ms of it pack + upload)   ({what})", flush=True)
        if range_only or a.no_search:
            del host, m
            continue
        # ---- the filtered search under these rows
        ix, V, terms, qseed = build(a.corpus, dev)
        if ix.post is not None:
            ix.drop_canonical()
        q = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in synth.queries_np(n_rows, V, terms, seed=qseed)]
        rows = torch.arange(n_rows, dtype=torch.int32, device=dev)
        flt = sparse_rx.DocFilter(out, n, ix.doc_base)
        res = ix.search_device(*q, a.k)
        line(f"search, {n_rows} queries x {terms} terms, k = {a.k}, unfiltered", timed(lambda: ix.search_device(*q, a.k, out=res), a.iters, a.warmup))
        allowed = flt.count()
        print(f"# the rows allow {int(allowed.min())} .. {int(allowed.max())} docs", flush=True)
        line("search under the field-built rows", timed(lambda: ix.search_device(*q, a.k, out=res, filter=flt, q_filter=rows), a.iters, a.warmup))

        def both():
            f = table.filter_device(**call, out=out)
            ix.search_device(*q, a.k, out=res, filter=f, q_filter=rows)
        line("builder + search", timed(both, a.iters, a.warmup))
        if h == n_rows:
            line("search under the from_masks rows", timed(lambda: ix.search_device(*q, a.k, out=res, filter=host, q_filter=rows), a.iters, a.warmup))
        else:
            print(f"# search under from_masks rows: the same bits in the same layout as the field-built rows (checked on {h} rows), so the same search", flush=True)
        ix.close()
        del host, m
    table.close()


if __name__ == "__main__":
    main()
