"""NumPy restatement of include/mx/sparse_rx_mx.h: the quantiser (value tables built from the format definitions, nearest with
ties to the even code through midpoints, integer scale arithmetic), the storage order, the dequantised values and the fp64
scores with the bound of the half index.  Nothing here calls the engine."""
import numpy as np

TYPES = {"mxfp8": 0, "mxfp4": 1}
EMAX = {"mxfp8": 8, "mxfp4": 2}
SIGN = {"mxfp8": 0x80, "mxfp4": 0x8}


def _values(ebits, mbits, bias, vmax):
    """the non-negative values of a minifloat by code, up to its finite maximum"""
    code = np.arange(1 << (ebits + mbits))
    e, m = code >> mbits, code & ((1 << mbits) - 1)
    v = np.where(e == 0, m * 2.0 ** (1 - bias - mbits), ((1 << mbits) + m) * 2.0 ** (e.astype(np.float64) - bias - mbits))
    return v[v <= vmax]


VALUES = {"mxfp8": _values(4, 3, 7, 448.0), "mxfp4": _values(2, 1, 1, 6.0)}  # 127 and 8 values, ascending = by code


def pad64(dim):
    return (dim + 63) // 64 * 64


def round_codes(a, dtype):
    """|v| (f64, any size) -> the code of the nearest value, ties to the even code; |v| is clamped to the maximum first"""
    vals = VALUES[dtype]
    a = np.minimum(a, vals[-1])
    mid = (vals[:-1] + vals[1:]) / 2
    lo, hi = np.searchsorted(mid, a, side="left"), np.searchsorted(mid, a, side="right")  # differ exactly on a midpoint
    return np.where(lo % 2 == 0, lo, hi)


def quantize(x, dtype, dim_pad=None):
    """f32[n, dim] -> (codes u8[n, dim_pad], scale codes u8[n, dim_pad / 32], flag)"""
    x = np.asarray(x, np.float32)
    n, dim = x.shape
    dim_pad = pad64(dim) if dim_pad is None else dim_pad
    xp = np.zeros((n, dim_pad), np.float32)
    xp[:, :dim] = x
    bad = ~np.isfinite(xp).all(axis=1)
    xp[bad] = 0.0
    b = xp.reshape(n, dim_pad // 32, 32)
    amax = (b.view(np.uint32) & 0x7FFFFFFF).max(axis=2).astype(np.int64)
    e = np.clip((amax >> 23) - 127 - EMAX[dtype], -127, 127)
    e[amax == 0] = 0
    v = np.ldexp(b.astype(np.float64), -e[:, :, None])  # exact in fp64
    q = round_codes(np.abs(v), dtype)
    q = np.where((q != 0) & (v < 0), q | SIGN[dtype], q)
    return q.reshape(n, dim_pad).astype(np.uint8), (e + 127).astype(np.uint8), int(bad.any())


def nbytes(dtype, n, dim_pad):
    t, ks = -(-n // 32), dim_pad // 64
    return t * 32 * dim_pad // (1 if dtype == "mxfp8" else 2) + t * -(-ks // 4) * 256


def pack(codes, scales, dtype):
    """the buffer of the header: codes in fragment order, then the scale dwords"""
    n, dim_pad = codes.shape
    t, ks = -(-n // 32), dim_pad // 64
    sg = -(-ks // 4)
    c = np.zeros((t * 32, dim_pad), np.uint8)
    c[:n] = codes
    if dtype == "mxfp4":  # [tile][k-step][half h][row][columns 32 h .. + 31], two to a byte
        c = c.reshape(t, 32, ks, 2, 32).transpose(0, 2, 3, 1, 4)
        c = c[..., 0::2] | (c[..., 1::2] << 4)
    else:  # [tile][k-step][half h][row][block b][columns 32 b + 16 h .. + 15]
        c = c.reshape(t, 32, ks, 2, 2, 16).transpose(0, 2, 4, 1, 3, 5)
    s = np.full((t * 32, sg * 4, 2), 127, np.uint8)
    s[:n, :ks] = scales.reshape(n, ks, 2)
    s = s.reshape(t, 32, sg, 4, 2).transpose(0, 2, 4, 1, 3)  # [tile][group][half][row][byte]
    out = np.concatenate([c.reshape(-1), s.reshape(-1)])
    assert out.size == nbytes(dtype, n, dim_pad)
    return out


def unpack(buf, dtype, n, dim_pad):
    t, ks = -(-n // 32), dim_pad // 64
    sg = -(-ks // 4)
    nb = t * 32 * dim_pad // (1 if dtype == "mxfp8" else 2)
    c = np.asarray(buf[:nb])
    if dtype == "mxfp4":
        c = np.stack([c & 15, c >> 4], axis=-1).reshape(t, ks, 2, 32, 32).transpose(0, 3, 1, 2, 4).reshape(t * 32, dim_pad)
    else:
        c = c.reshape(t, ks, 2, 32, 2, 16).transpose(0, 3, 1, 4, 2, 5).reshape(t * 32, dim_pad)
    s = np.asarray(buf[nb:]).reshape(t, sg, 2, 32, 4).transpose(0, 3, 1, 4, 2).reshape(t * 32, sg * 8)
    return c[:n], s[:n, : 2 * ks]


def dequant(codes, scales, dtype):
    c = codes.astype(np.int64)
    v = VALUES[dtype][c & (SIGN[dtype] - 1)] * np.where(c & SIGN[dtype], -1.0, 1.0)
    return v * np.repeat(np.ldexp(1.0, scales.astype(np.int64) - 127), 32, axis=1)


def operands(q, emb, dtype):
    """the dequantised MXFP8 queries and `dtype` docs, f64, padded"""
    dim_pad = pad64(emb.shape[1])
    return dequant(*quantize(q, "mxfp8", dim_pad)[:2], "mxfp8"), dequant(*quantize(emb, dtype, dim_pad)[:2], dtype)


def exact_scores(qd, dd):
    return qd @ dd.T


def tol(qd, dd):
    """dim_pad * 2^-22 * sum |q_i d_i|: each product (two significands of at most 4 bits, two powers of two) is exact in fp32; each
    of at most dim_pad accumulations loses at most one fp32 ulp (2^-23 relative) of a partial sum bounded by the absolute sum;
    doubled, as the half index's bound is"""
    return qd.shape[1] * 2.0 ** -22 * (np.abs(qd) @ np.abs(dd).T)
