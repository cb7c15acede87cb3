"""What facet counts cost: ``srx_facet_counts`` and ``srx_facet_counts_lists`` next to two other routes to the
same numbers, measured in the same session:

  a. torch ops on the same GPU: unpack the row's bits, then ``torch.bincount(codes[mask], minlength=n_bins)`` per row, and one
     batched ``scatter_add`` over a chunk of rows; the faster of the two is reported and named;
  b. the host route: the row copied back, NumPy ``unpackbits`` + ``np.bincount`` (wall clock).

The torch route runs on ``--slow-rows`` rows at most, the host route on 2, both scaled to the row count; the tool asserts that
all routes give equal counts before it times them.  ``srx_filter_count`` is timed on the same rows: a sparse row should cost about that, not a dense row's
price.  Shapes: an I32 category column of 64 and of 4 096 values, uniform and skewed (about 90 % of the docs in one value);
1, 32 and 1 000 rows of density 0.5 and 2^-10; one EDGES case on an F32 column with 16 bins; one LABELS case with 12 labels;
the list form at 1 024 lists x m = 128 and 1 024.  Each number is the median (min .. max) of ``--iters`` hipEvent-timed
repetitions after ``--warmup``.

    python tools/bench_facets.py [--docs 100000 10000000] [--rows 1 32 1000] [--iters 20] [--warmup 5] [--out profiles/facets.log]
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparse_rx  # noqa: E402
from sparse_rx import _capi  # noqa: E402
from sparse_rx.fields import FieldTable, HostColumn  # noqa: E402
from sparse_rx.filter import DocFilter, filter_words  # noqa: E402
from bench_filtered import timed  # noqa: E402

DEV = torch.device("cuda:0")
OUT = None


def say(text):
    print(text, flush=True)
    if OUT is not None:
        OUT.write(text + "\n")
        OUT.flush()


def ms(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def random_rows(n_rows, n_docs, dense, seed):
    """Filter rows of density 0.5 (random words) or 2^-10 (the AND of ten random words), tail bits and padding words 0"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    words = filter_words(n_docs)
    bits = torch.randint(-2 ** 31, 2 ** 31, (n_rows, words), dtype=torch.int64, device=DEV, generator=g).to(torch.int32)
    if not dense:
        for _ in range(9):
            bits &= torch.randint(-2 ** 31, 2 ** 31, (n_rows, words), dtype=torch.int64, device=DEV, generator=g).to(torch.int32)
    full = torch.from_numpy(sparse_rx.filter.pack_masks(np.ones(n_docs, dtype=bool)).view(np.int32).copy()).to(DEV)
    bits &= full
    return DocFilter(bits.contiguous(), n_docs)


def unpack(row_words, n_docs):
    shifts = torch.arange(32, device=DEV, dtype=torch.int32)
    return ((row_words[:, None] >> shifts) & 1).to(torch.bool).reshape(-1)[:n_docs]


def torch_bincount(flt, rows, codes, n_bins, out):
    for i, r in enumerate(rows):
        out[i] = torch.bincount(codes[unpack(flt.bits[r], flt.n_docs)], minlength=n_bins)[:n_bins]
    return out


def torch_scatter(flt, rows, codes, n_bins, out, chunk=4):
    out.zero_()
    shifts = torch.arange(32, device=DEV, dtype=torch.int32)
    for r0 in range(0, len(rows), chunk):
        sel = torch.as_tensor(rows[r0: r0 + chunk], device=DEV)
        mask = ((flt.bits[sel][:, :, None] >> shifts) & 1).reshape(len(sel), -1)[:, : flt.n_docs].to(torch.int64)
        out[r0: r0 + len(sel)].scatter_add_(1, codes[None, :].expand(len(sel), -1), mask)
    return out


def host_route(flt, rows, codes_np, n_bins):
    t0 = time.perf_counter()
    out = np.zeros((len(rows), n_bins), dtype=np.int64)
    for i, r in enumerate(rows):
        w = flt.bits[r].cpu().numpy()
        mask = np.unpackbits(w.view(np.uint8), bitorder="little")[: flt.n_docs].astype(bool)
        out[i] = np.bincount(codes_np[mask], minlength=n_bins)[:n_bins]
    return out, (time.perf_counter() - t0) * 1e3


def zipf_codes(rng, n, n_values):
    """About 90 % of the docs in value 3, the rest uniform"""
    return np.where(rng.random(n) < 0.9, 3, rng.integers(0, n_values, n)).astype(np.int32)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, nargs="+", default=[100_000, 10_000_000])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 32, 1000])
    ap.add_argument("--slow-rows", type=int, default=8, help="rows the torch and host routes run on (scaled to the row count)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT = open(a.out, "w")
    L = _capi.lib()
    stream = lambda: torch.cuda.current_stream(DEV).cuda_stream
    say(f"# {torch.cuda.get_device_name(0)}; median (min .. max) ms of {a.iters} hipEvent-timed repetitions after {a.warmup} warm-up; torch route on "
        f"<= {a.slow_rows} rows and host route on <= 2, scaled; TB/s = (row words + the column once) / time, roofline 8 TB/s")
    for n in a.docs:
        rng = np.random.default_rng(n)
        cols = {}
        for n_values in (64, 4096):
            names = [f"v{i:04d}" for i in range(n_values)]
            cols[f"uni{n_values}"] = HostColumn("category", rng.integers(0, n_values, n).astype(np.int32), None, names)
            cols[f"zipf{n_values}"] = HostColumn("category", zipf_codes(rng, n, n_values), None, names)
        cols["price"] = (rng.random(n) * 100).astype(np.float32)
        cols["tags"] = HostColumn("set", rng.integers(0, 1 << 12, n, dtype=np.int64) & rng.integers(0, 1 << 12, n, dtype=np.int64), None,
                                  [f"t{i:02d}" for i in range(12)])
        codes_np = {k: c.data.copy() for k, c in cols.items() if isinstance(c, HostColumn) and c.kind == "category"}
        table = FieldTable.from_columns(cols, device=DEV)
        words = filter_words(n)
        say(f"\n## {n} docs, {words * 4} bytes per row")
        for n_rows in a.rows:
            for dense in (True, False):
                flt = random_rows(n_rows, n, dense, seed=n_rows + int(dense))
                q = torch.arange(n_rows, dtype=torch.int32, device=DEV)
                allowed = torch.empty(n_rows, dtype=torch.int32, device=DEV)
                t_cnt = timed(lambda: L.srx_filter_count(0, flt.bits.data_ptr(), n_rows, n, allowed.data_ptr(), stream()), a.iters, a.warmup)
                counted = int(allowed.sum().item())
                say(f"\n{n_rows} rows of density {'0.5' if dense else '2^-10'}: {counted} docs counted; srx_filter_count on these rows {ms(t_cnt)}")
                slow = list(range(min(n_rows, a.slow_rows)))
                scale = n_rows / len(slow)
                base = {}
                for name in ("uni64", "zipf64", "uni4096", "zipf4096"):
                    n_bins = len(cols[name].dictionary)
                    codes = table._tensors[name][0].to(torch.int64)
                    counts, extra = table.facet_device(name, None, flt, q)
                    ref_b = torch_bincount(flt, slow, codes, n_bins, torch.zeros((len(slow), n_bins), dtype=torch.int64, device=DEV)).clone()
                    ref_s = torch_scatter(flt, slow, codes, n_bins, torch.zeros((len(slow), n_bins), dtype=torch.int64, device=DEV)).clone()
                    ref_h, _ = host_route(flt, slow[:2], codes_np[name], n_bins)
                    torch.cuda.synchronize()
                    assert torch.equal(counts[: len(slow)].to(torch.int64), ref_b) and torch.equal(ref_b, ref_s), "the torch routes and the kernel disagree"
                    assert np.array_equal(counts[:2].cpu().numpy(), ref_h[: len(counts[:2])]), "the host route and the kernel disagree"
                    assert torch.equal(extra[:, 2], allowed) and int(extra[:, :2].sum().item()) == 0
                    t = timed(lambda: table.facet_device(name, None, flt, q), a.iters, a.warmup)
                    buf = torch.zeros((len(slow), n_bins), dtype=torch.int64, device=DEV)
                    tb = timed(lambda: torch_bincount(flt, slow, codes, n_bins, buf), a.iters, a.warmup)
                    ts = timed(lambda: torch_scatter(flt, slow, codes, n_bins, buf), a.iters, a.warmup)
                    best, which = (tb, "bincount per row") if tb[0] <= ts[0] else (ts, "batched scatter_add")
                    _, th = host_route(flt, slow[:2], codes_np[name], n_bins)
                    moved = n_rows * words * 4 + n * 4
                    base[name] = t[0]
                    say(f"  {name:9s} kernel {ms(t)}  {moved / t[0] / 1e9:6.3f} TB/s  {counted / t[0] / 1e6:8.2f} G docs/s | torch ({which}) "
                        f"{best[0] * scale:10.3f} ms = {best[0] * scale / t[0]:7.1f}x | host {th / min(2, len(slow)) * n_rows:10.1f} ms | "
                        f"vs srx_filter_count {t[0] / t_cnt[0]:6.1f}x")
                for n_values in (64, 4096):
                    say(f"  skewed / uniform at {n_values} values: {base[f'zipf{n_values}'] / base[f'uni{n_values}']:.2f}x")
                if n_rows == a.rows[-1] or n_rows == 32:
                    edges = {"edges": [float(e) for e in np.linspace(0, 100, 17)]}
                    t = timed(lambda: table.facet_device("price", edges, flt, q), a.iters, a.warmup)
                    c, e = table.facet_device("price", edges, flt, q)
                    mask0 = unpack(flt.bits[0], n)
                    want = torch.bincount(torch.bucketize(table._tensors["price"][0][mask0], torch.as_tensor(edges["edges"], dtype=torch.float32, device=DEV),
                                                          right=True) - 1, minlength=17)[:16]
                    assert torch.equal(c[0].to(torch.int64), want), "the EDGES case disagrees with torch.bucketize"
                    say(f"  price     kernel {ms(t)}  EDGES, F32 column, 16 bins  {counted / t[0] / 1e6:8.2f} G docs/s")
                    t = timed(lambda: table.facet_device("tags", None, flt, q), a.iters, a.warmup)
                    c, e = table.facet_device("tags", None, flt, q)
                    tags0 = table._tensors["tags"][0][mask0]
                    want = torch.stack([((tags0 >> i) & 1).sum() for i in range(12)])
                    assert torch.equal(c[0].to(torch.int64), want), "the LABELS case disagrees with torch"
                    say(f"  tags      kernel {ms(t)}  LABELS, 12 labels          {counted / t[0] / 1e6:8.2f} G docs/s")
                del flt
        # ---- the list form
        for m in (128, 1024):
            nq = 1024
            g = torch.Generator(device=DEV)
            g.manual_seed(m)
            doc = torch.randint(0, n, (nq, m), dtype=torch.int64, device=DEV, generator=g).to(torch.int32)
            cnt = torch.full((nq,), m, dtype=torch.int32, device=DEV)
            for name in ("uni64", "zipf64", "uni4096", "zipf4096"):
                n_bins = len(cols[name].dictionary)
                codes = table._tensors[name][0].to(torch.int64)
                ones = torch.ones((nq, m), dtype=torch.int64, device=DEV)

                def torch_lists():
                    return torch.zeros((nq, n_bins), dtype=torch.int64, device=DEV).scatter_add_(1, codes[doc.long()], ones)
                c, e = table.facet_lists_device(name, doc, cnt)
                torch.cuda.synchronize()
                assert torch.equal(c.to(torch.int64), torch_lists()), "the list form disagrees with torch"
                t = timed(lambda: table.facet_lists_device(name, doc, cnt), a.iters, a.warmup)
                tt = timed(torch_lists, a.iters, a.warmup)
                say(f"lists 1024 x {m:4d}  {name:9s} kernel {ms(t)}  {nq * m / t[0] / 1e6:8.2f} G docs/s | torch (gather + scatter_add) {ms(tt)} = {tt[0] / t[0]:6.1f}x")
        table.close()
    if OUT is not None:
        OUT.close()


if __name__ == "__main__":
    main()
