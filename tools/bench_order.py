"""What ordering by a field costs: ``srx_order_topk`` and ``srx_order_lists`` next to the torch route to the same
values on the same GPU, measured in the same session:

  rows   unpack the row's bits, ``torch.where`` the column to a sentinel outside the set, ``torch.topk``;
  lists  gather the values, a stable ``torch.sort``, gather the docs.

``torch.topk`` does not order ties, so the tool asserts equal KEY VALUES (and equal docs for the list form) before it times.  The
torch row route is ONE batched call over all rows (chunks of rows of at most 2^28 docs each, so that the unpacked block stays
below 2 GiB of int64) and is timed in full; the line says how many chunks it took.  Shapes, each over an int64 column of random
values: 1 000 rows of density 0.5 at 100 k and 10 M docs, 1 000 rows of density 2^-10 and one dense row at 10 M docs, k = 10 and
1 024; the list form at 1 024 lists of m = 128 / 1 024 / 2 048.  Each number is the median (min .. max) of ``--iters``
hipEvent-timed repetitions after ``--warmup``.

    python tools/bench_order.py [--iters 20] [--warmup 5] [--out profiles/order.log]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparse_rx  # noqa: F401,E402
from sparse_rx import _capi  # noqa: E402
from sparse_rx.fields import FieldTable  # noqa: E402
from sparse_rx.filter import filter_words  # noqa: E402
from bench_facets import random_rows  # noqa: E402
from bench_filtered import timed  # noqa: E402

DEV = torch.device("cuda:0")
OUT = None
I64_MIN = -(2 ** 63)


def say(text):
    print(text, flush=True)
    if OUT is not None:
        OUT.write(text + "\n")
        OUT.flush()


def ms(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def torch_rows(flt, col, k, chunk):
    """descending, valueless docs do not occur: the k largest values of every row, `chunk` rows per batched where + topk"""
    shifts = torch.arange(32, device=DEV, dtype=torch.int32)
    out = []
    for r0 in range(0, flt.bits.shape[0], chunk):
        mask = ((flt.bits[r0: r0 + chunk][:, :, None] >> shifts) & 1).to(torch.bool).reshape(-1, flt.bits.shape[1] * 32)[:, : flt.n_docs]
        out.append(torch.topk(torch.where(mask, col[None, :], I64_MIN), k, dim=1).values)
    return torch.cat(out)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT = open(a.out, "w")
    say(f"# {torch.cuda.get_device_name(0)}; median (min .. max) ms of {a.iters} hipEvent-timed repetitions after {a.warmup} warm-up (the torch row route over more than 2^30 "
        f"docs: 3 after 1); TB/s = (row words + 8 bytes per doc of the set) / time, roofline 8 TB/s")
    for n, shapes in ((100_000, [(1000, True)]), (10_000_000, [(1000, True), (1000, False), (1, True)])):
        rng = np.random.default_rng(n)
        table = FieldTable.from_columns({"stamp": rng.integers(-2 ** 62, 2 ** 62, n)}, device=DEV)
        col = table._tensors["stamp"][0]
        words = filter_words(n)
        say(f"\n## {n} docs, int64 column, {words * 4} bytes per row")
        for n_rows, dense in shapes:
            flt = random_rows(n_rows, n, dense, seed=n_rows + int(dense))
            q = torch.arange(n_rows, dtype=torch.int32, device=DEV)
            for k in (10, 1024):
                doc, key, extra = table.top_by_device("stamp", k, "desc", "last", flt, q)
                chunk = max(1, min(n_rows, 2 ** 28 // n))
                ref = torch_rows(flt, col, k, chunk)
                torch.cuda.synchronize()
                in_set = int(extra[:, 2].sum().item())
                count = torch.minimum(extra[:, 2], torch.tensor(k, device=DEV, dtype=torch.int32))
                live = torch.arange(k, device=DEV)[None, :] < count[:, None]
                assert torch.equal(extra[:, 0], count) and torch.equal(key[live], ref[live]), "the torch route and the kernel disagree"
                t = timed(lambda: table.top_by_device("stamp", k, "desc", "last", flt, q), a.iters, a.warmup)
                tt = timed(lambda: torch_rows(flt, col, k, chunk), a.iters if n_rows * n <= 2 ** 30 else 3, a.warmup if n_rows * n <= 2 ** 30 else 1)
                moved = n_rows * words * 4 + in_set * 8
                segs, ws = _capi.order_plan(n, n_rows, k)
                say(f"{n_rows:5d} rows of density {'0.5  ' if dense else '2^-10'} k = {k:4d}: kernel {ms(t)}  {moved / t[0] / 1e9:6.3f} TB/s  "
                    f"{in_set / t[0] / 1e6:8.2f} G docs/s | torch (batched where + topk, {-(-n_rows // chunk)} call{'s' if n_rows > chunk else ''} of {chunk} rows) "
                    f"{ms(tt)} = {tt[0] / t[0]:7.1f}x | {segs} segments, workspace {ws / 2 ** 20:.1f} MiB")
            del flt
        if n == 10_000_000:
            for m in (128, 1024, 2048):
                nq = 1024
                g = torch.Generator(device=DEV)
                g.manual_seed(m)
                doc = torch.randint(0, n, (nq, m), dtype=torch.int64, device=DEV, generator=g).to(torch.int32)
                score = torch.rand((nq, m), device=DEV, generator=g)

                def torch_lists():
                    order = torch.sort(col[doc.long()], dim=1, descending=True, stable=True).indices
                    return torch.gather(doc, 1, order), torch.gather(score, 1, order)
                d, s, key, extra = table.sort_lists_device("stamp", doc, score, None, m, "desc", "last")
                rd, rs = torch_lists()
                torch.cuda.synchronize()
                assert torch.equal(d, rd) and torch.equal(s, rs), "the list form disagrees with torch"
                t = timed(lambda: table.sort_lists_device("stamp", doc, score, None, m, "desc", "last"), a.iters, a.warmup)
                tt = timed(torch_lists, a.iters, a.warmup)
                say(f"lists 1024 x {m:4d}: kernel {ms(t)}  {nq * m / t[0] / 1e6:8.2f} G docs/s | torch (gather + stable sort + gathers) {ms(tt)} = {tt[0] / t[0]:6.1f}x")
        table.close()
    if OUT is not None:
        OUT.close()


if __name__ == "__main__":
    main()
