"""NumPy restatement of the device quantisers' contract (include/sparse_rx_quant.h), written from the
header: the four formulas of the reference (rag_system/core/retriever_registry.py:435-462, 482-491, 555) in fp32, one rounded
operation per line, plus the results the header defines where the reference divides by zero or casts NaN.  Every function takes
f32[n, dim] and returns arrays padded with zeros to ``dim_pad`` columns (``None``: ``dim``) and the flag word."""
import numpy as np

F = np.float32
NONFINITE, DEGENERATE = 1, 2
DIMS = (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024)


def pad_i8(dim):
    return next(d for d in DIMS if d >= dim)


def pad_u8(dim):
    return (dim + 63) // 64 * 64


def _f32(e):
    e = np.asarray(e)
    assert e.dtype == np.float32 and e.ndim == 2 and e.shape[1] >= 1
    return e


def _padded(a, dim_pad):
    out = np.zeros((a.shape[0], dim_pad or a.shape[1]), a.dtype)
    out[:, : a.shape[1]] = a
    return out


def _flag(bad, zero=None):
    return (NONFINITE if bad.any() else 0) | (DEGENERATE if zero is not None and zero.any() else 0)


def _i8(e, query, dim_pad):
    e = _f32(e)
    bad = ~np.isfinite(e).all(axis=1)
    x = np.where(bad[:, None], F(0), e)            # a flagged row's codes are 0 whatever it holds
    a = np.abs(x)
    m = np.max(a, axis=1)
    zero = (m == 0) & ~bad if query else np.zeros_like(bad)
    s = m if query else np.maximum(m, F(1e-8))
    with np.errstate(all="ignore"):
        t = x / s[:, None]
        t = t * F(127.0)
        t = np.rint(t)
    t[bad | zero] = 0
    codes = t.astype(np.int32).astype(np.int8)
    if query:
        with np.errstate(all="ignore"):
            scale = s / F(127.0)
        scale[bad | zero] = 0
    else:
        scale = s.copy()
        scale[bad] = F(1e-8)
    assert t.dtype == np.float32 and scale.dtype == np.float32
    return _padded(codes, dim_pad), scale, _flag(bad, zero)


def i8_rows(e, dim_pad=None):
    """-> (i8[n, dim_pad], f32[n] scales, flag)"""
    return _i8(e, False, dim_pad)


def i8_queries(q, dim_pad=None):
    """-> (i8[nq, dim_pad], f32[nq] query scales = max|x| / 127, flag)"""
    return _i8(q, True, dim_pad)


def _u8(e, query, dim_pad):
    e = _f32(e)
    bad = ~np.isfinite(e).all(axis=1)
    x = np.where(bad[:, None], F(0), e)
    mn = np.min(x, axis=1)
    mx = np.max(x, axis=1)
    with np.errstate(all="ignore"):
        d = mx - mn
        over = ~np.isfinite(d)                      # max - min overflows
        bad = bad | over
        sc = d / F(255.0)
        if not query:
            sc = np.maximum(sc, F(1e-8))
        zero = (sc == 0) & ~bad if query else np.zeros_like(bad)
        t = x - mn[:, None]
        t = t / sc[:, None]
        t = np.rint(t)
    t[bad | zero] = 0
    codes = t.astype(np.int32).astype(np.uint8)
    sc, mn = sc.copy(), mn.copy()
    sc[bad] = F(0) if query else F(1e-8)
    mn[bad] = 0
    sc[zero] = 0
    assert t.dtype == np.float32 and sc.dtype == np.float32 and mn.dtype == np.float32
    return codes, sc, mn, _flag(bad, zero)


def u8_rows(e, dim_pad=None):
    """-> (u8[n, dim_pad], f32[2 n] = all scales then all minima, flag)"""
    codes, sc, mn, flag = _u8(e, False, dim_pad)
    return _padded(codes, dim_pad), np.concatenate([sc, mn]), flag


def u8_queries(q, dim_pad=None):
    """-> (u8[nq, dim_pad], f32[nq, 2] = (scale, min), de-quantised f32[nq, dim_pad], flag)"""
    codes, sc, mn, flag = _u8(q, True, dim_pad)
    deq = codes.astype(np.float32)
    deq = deq * sc[:, None]
    deq = deq + mn[:, None]
    assert deq.dtype == np.float32
    return _padded(codes, dim_pad), np.stack([sc, mn], axis=1), _padded(deq, dim_pad), flag


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def make_rows(seed, n, dim, degenerate=True, denormal=True):
    """f32[n, dim] test rows: magnitudes from 1e-9 to 1e4, then (as far as n allows) the rows the contract names -- 1e-9 (the
    clamp), 1e30, values that land on .5 before rounding in either scheme, -0.0 next to positive values, denormals, and with
    ``degenerate`` a row of zeros and a constant row (degenerate as QUERIES, plain rows of a corpus)."""
    rng = np.random.default_rng(seed)
    e = (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-9, 4, (n, 1))).astype(np.float32)
    special = []
    special.append((rng.standard_normal(dim) * 1e-9).astype(np.float32))
    special.append((rng.standard_normal(dim) * 1e30).astype(np.float32))
    h = rng.integers(-127, 127, dim).astype(np.float32) + F(0.5)       # i8: max |x| = 127 -> x / 127 * 127 near k + .5
    h[rng.integers(0, dim)] = 127
    special.append(h)
    h = rng.integers(0, 255, dim).astype(np.float32) + F(0.5)          # u8: min 0, max 255 -> scale 1, codes round half to even
    h[rng.integers(0, dim)] = 0
    if dim > 1:
        h[(int(np.argmin(h)) + 1) % dim] = 255
    special.append(h)
    z = np.abs(rng.standard_normal(dim)).astype(np.float32) + F(0.1)
    z[::2] = -0.0                                                      # -0.0 is the minimum; no +0 in the row
    special.append(z)
    if denormal:
        special.append((rng.integers(-500, 500, dim) * 1.4e-45).astype(np.float32))
    if degenerate:
        special.append(np.zeros(dim, np.float32))
        special.append(np.full(dim, 0.37, np.float32))
    if dim == 1 and not degenerate:
        special = [row for row in special if row[0] != 0]              # a 1-d zero is a degenerate query
    for i, row in enumerate(special):
        if 2 * i + 1 < n:
            e[2 * i + 1] = row
        elif i < n and n <= 2:
            e[i] = row
    return e
