"""Dev bench of the device quantisers (include/sparse_rx_quant.h): what building the resident dense index from f32 embeddings
costs on the device next to the host route to the same index, and what quantising a query batch costs next to the host loop
and to the INT8 search it feeds.  One process, one stream, device events around each call, warmed up.

  python tools/bench_dense_build.py [--docs N] [--dim D] [--nq N] [--iters N]

  * the fused quantise (+ pack) kernels over docs x dim f32 on the device: median, p10 / p90 and bytes moved / time (4 bytes
    read and 1 written per element, plus the scale table) next to the HBM peak and to a plain device copy of the same matrix;
  * the host route to the same resident index: NumPy quantisation (in row chunks of 64 MB), then upload, zero-pad and pack
    (the index constructor); timed once each, wall clock around a synchronise;
  * query quantisation of nq x dim on the device against the per-query host loop, next to the INT8 search of the batch.
Every run checks the device results against the host functions bit for bit and fails if they differ."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import sparse_rx
from sparse_rx import dense

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nq", type=int, default=1024)
ap.add_argument("--iters", type=int, default=100)
args = ap.parse_args()
n, dim, nq, iters = args.docs, args.dim, args.nq, args.iters
WARM, HBM_PEAK = 10, 8.0e12
dev = torch.device("cuda:0")


def stats(x):
    x = np.sort(np.asarray(x))
    return float(np.median(x)), f"median {np.median(x):.4f} ms (p10 {x[len(x) // 10]:.4f}, p90 {x[(9 * len(x)) // 10]:.4f}, n={len(x)})"


def timed(fn, reps=iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for it in range(-WARM, reps):
        a, b = ev[max(it, 0)]
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def host_chunks(fn, e):
    """A host quantiser over row chunks of <= 64 MB (bounded temporaries), results concatenated."""
    rows = max(1, (64 << 20) // (4 * e.shape[1]))
    parts = [fn(e[lo: lo + rows]) for lo in range(0, e.shape[0], rows)]
    return np.concatenate([p[0] for p in parts]), [p[1] for p in parts]


g = torch.Generator(device=dev)
g.manual_seed(20252)
emb = torch.randn((n, dim), generator=g, device=dev, dtype=torch.float32)
emb *= torch.exp(torch.randn((n, 1), generator=g, device=dev))  # rows of different magnitudes
queries = torch.randn((nq, dim), generator=g, device=dev, dtype=torch.float32)
dim_pad, dim_pad_u8 = dense._pad_dim(dim), dense._pad64(dim, "uint8")
print(f"dense build bench on {torch.cuda.get_device_name(0)}: {n} x {dim} f32 ({n * dim * 4 / 2 ** 30:.2f} GiB), {nq} queries, {iters} timed "
      f"iterations after {WARM} warm-up", flush=True)

# ---- the kernels ----------------------------------------------------------------------------------------------------------
L = sparse_rx._capi.lib()
flag = torch.zeros(1, dtype=torch.int32, device=dev)
packed = torch.empty(L.srx_dense_packed_bytes(n, dim_pad), dtype=torch.int8, device=dev)
rowmajor = torch.empty((n, dim_pad), dtype=torch.int8, device=dev)
scales = torch.empty(n, dtype=torch.float32, device=dev)
u8 = torch.empty((n, dim_pad_u8), dtype=torch.uint8, device=dev)
table = torch.empty(2 * n, dtype=torch.float32, device=dev)
copy_dst = torch.empty_like(emb)
runs = (("srx_dense_quantize_i8, fragment order", lambda: dense._quantize_device("srx_dense_quantize_i8", emb, dim_pad, (packed, scales), flag, 0, n, 1),
         n * (4 * dim + dim_pad + 4)),
        ("srx_dense_quantize_i8, row-major    ", lambda: dense._quantize_device("srx_dense_quantize_i8", emb, dim_pad, (rowmajor, scales), flag, 0, n, 0),
         n * (4 * dim + dim_pad + 4)),
        ("srx_dense_quantize_u8               ", lambda: dense._quantize_device("srx_dense_quantize_u8", emb, dim_pad_u8, (u8, table), flag, 0, n),
         n * (4 * dim + dim_pad_u8 + 8)),
        ("plain device copy of the f32 matrix ", lambda: copy_dst.copy_(emb), 2 * n * dim * 4))
for name, fn, nbytes in runs:
    med, text = timed(fn)
    rate = nbytes / (med * 1e-3)
    print(f"  {name}  {text}; {nbytes / 1e9:.2f} GB moved -> {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of the {HBM_PEAK / 1e12:.0f} TB/s peak",
          flush=True)
del copy_dst
assert flag.item() == 0

# ---- the host route to the same resident index, and the bit check ---------------------------------------------------------------
emb_h, t_down = wall(lambda: emb.cpu().numpy())
for scheme, fn, cls, dev_tensors in (("symmetric INT8", sparse_rx.quantize_symmetric, sparse_rx.DenseInt8Index, (packed, scales)),
                                     ("asymmetric uint8", sparse_rx.quantize_asymmetric, sparse_rx.DenseUint8Index, (u8, table))):
    t = time.perf_counter()
    codes, parts = host_chunks(fn, emb_h)
    tab = np.concatenate(parts) if cls is sparse_rx.DenseInt8Index else np.concatenate([np.concatenate([p[: len(p) // 2] for p in parts]),
                                                                                        np.concatenate([p[len(p) // 2:] for p in parts])])
    t_quant = (time.perf_counter() - t) * 1e3
    ix, t_up = wall(lambda: cls(codes, tab, device=dev))
    same = bool(torch.equal(ix.corpus, dev_tensors[0]) and torch.equal(ix.scales, dev_tensors[1]))
    ix2, t_dev_host = wall(lambda: cls.from_embeddings(emb_h, device=dev))
    same2 = bool(torch.equal(ix2.corpus, ix.corpus) and torch.equal(ix2.scales, ix.scales))
    print(f"  host route, {scheme}: NumPy quantise {t_quant:.0f} ms + upload, pad{', pack' if cls is sparse_rx.DenseInt8Index else ''} {t_up:.0f} ms; "
          f"from_embeddings of the same host array (chunked f32 upload + kernel) {t_dev_host:.0f} ms; device corpus and scales "
          f"{'equal the host route bit for bit' if same and same2 else 'DIFFER'}", flush=True)
    assert same and same2, "device and host quantisers disagree"
    del ix, ix2, codes
print(f"  (copying the f32 matrix device -> host took {t_down:.0f} ms)")

# ---- the query batch ---------------------------------------------------------------------------------------------------------
ix = sparse_rx.DenseInt8Index.from_embeddings(emb, device=dev)
q_h = queries.cpu().numpy()
_, text = timed(lambda: sparse_rx.quantize_queries_symmetric_device(queries))
print(f"  query quantisation {nq} x {dim}, device (allocations included)  {text}")
_, text = timed(lambda: sparse_rx.quantize_queries_asymmetric_device(queries))
print(f"  the same, asymmetric (codes, pairs and the de-quantised block)    {text}")
host_ms = []
for _ in range(5):
    t = time.perf_counter()
    qq = [sparse_rx.quantize_query_symmetric(e) for e in q_h]
    qi, qs = np.stack([a for a, _ in qq]), np.array([b for _, b in qq], dtype=np.float32)
    host_ms.append((time.perf_counter() - t) * 1e3)
print(f"  the host loop of quantize_query_symmetric + stack                 median {np.median(host_ms):.2f} ms (min {min(host_ms):.2f}, n=5)")
dq, dqs, qflag = sparse_rx.quantize_queries_symmetric_device(queries)
same = bool(np.array_equal(dq.cpu().numpy(), qi) and np.array_equal(dqs.cpu().numpy().view(np.uint32), qs.view(np.uint32)) and qflag.item() == 0)
print(f"  device query codes and scales {'equal the host loop bit for bit' if same else 'DIFFER'}")
assert same
dqi, dqs2 = torch.as_tensor(qi, device=dev), torch.as_tensor(qs, device=dev)
_, text = timed(lambda: ix.search_device(dqi, dqs2, 10), reps=20)
print(f"  srx_dense_search_i8_packed of the batch, k = 10                   {text}")
_, text = timed(lambda: ix.search_f32_device(queries, 10), reps=20)
print(f"  search_f32_device (quantise + search), k = 10                     {text}")
