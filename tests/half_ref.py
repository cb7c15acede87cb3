"""NumPy restatement of include/sparse_rx_half.h, written from the header: the two roundings, the fragment-order layout, what
the conversion writes, the exact scores of the rounded operands and the derived error bound.  Never calls the engine; the
ranking is tests/parity.py's dense_topk_rows, imported by the tests and not modified."""
import numpy as np

TYPES = {"f16": 0, "bf16": 1}  # srx_half_type


# ---- the two roundings: f32 -> 16-bit codes, round to nearest even, subnormals included -----------------------------------
def round_f16(x):
    """NumPy's own conversion (IEEE round-to-nearest-even; overflow gives inf)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def round_bf16(x):
    """Integer arithmetic on the bit pattern: add 0x7FFF plus the lowest kept bit, keep the upper half.  inf stays inf, a NaN
    stays a (quiet) NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nonfinite = (u & 0x7F800000) == 0x7F800000
    nan = nonfinite & ((u & 0x007FFFFF) != 0)
    r = np.where(nonfinite, (u >> 16) | np.where(nan, np.uint64(0x40), np.uint64(0)), r)
    return r.astype(np.uint16)


def round_codes(x, dtype):
    return round_f16(x) if dtype == "f16" else round_bf16(x)


def to_f32(codes, dtype):
    """The value of every 16-bit code, as float32 (exact for both types)."""
    c = np.ascontiguousarray(codes, dtype=np.uint16)
    return c.view(np.float16).astype(np.float32) if dtype == "f16" else (c.astype(np.uint32) << 16).view(np.float32)


def finite(codes, dtype):
    c = np.asarray(codes, dtype=np.uint16)
    return (c & 0x7C00) != 0x7C00 if dtype == "f16" else (c & 0x7F80) != 0x7F80


def convert(emb, dtype, dim_pad):
    """What srx_dense_convert_half stores for f32[n, dim] rows: (u16[n, dim_pad] codes, flag).  Columns dim .. dim_pad - 1 are
    zeros; a row with a value whose rounding is not finite is all zeros and sets flag bit 0."""
    e = np.asarray(emb, dtype=np.float32)
    n, dim = e.shape
    codes = np.zeros((n, dim_pad), np.uint16)
    codes[:, :dim] = round_codes(e, dtype)
    bad = ~finite(codes, dtype).all(axis=1)
    codes[bad] = 0
    return codes, int(bad.any())


# ---- the fragment-order layout ----------------------------------------------------------------------------------------------
def half_bytes(n_rows, dim_pad):
    return (n_rows + 31) // 32 * 32 * dim_pad * 2


def byte_offset(r, c, dim_pad):
    """The header's formula for element (row r, column c)."""
    ks = dim_pad // 16
    return ((((r >> 5) * ks + (c >> 4)) * 64 + (r & 31) + 32 * ((c >> 3) & 1)) * 8 + (c & 7)) * 2


def pack(codes):
    """u16[n, dim_pad] row-major -> the u16 buffer of the whole corpus (rows past n in the last tile are zeros)."""
    c = np.asarray(codes, dtype=np.uint16)
    n, dim_pad = c.shape
    tiles, ks = (n + 31) // 32, dim_pad // 16
    full = np.zeros((tiles * 32, dim_pad), np.uint16)
    full[:n] = c
    t = full.reshape(tiles, 32, ks, 2, 8)  # [tile][row][k-step][half][element]
    return np.ascontiguousarray(t.transpose(0, 2, 3, 1, 4)).reshape(-1)  # [tile][k-step][half][row][element]: lane = row + 32 half


def unpack(packed, n, dim_pad):
    ks = dim_pad // 16
    t = np.asarray(packed).view(np.uint16).reshape(-1, ks, 2, 32, 8)
    return np.ascontiguousarray(t.transpose(0, 3, 1, 2, 4)).reshape(-1, dim_pad)[:n]


# ---- scores -----------------------------------------------------------------------------------------------------------------
def exact_scores(q_codes, d_codes, dtype):
    """fp64 dot products of the rounded operands: f64[nq, n]."""
    return to_f32(q_codes, dtype).astype(np.float64) @ to_f32(d_codes, dtype).astype(np.float64).T


def abs_scores(q_codes, d_codes, dtype):
    """sum_i |q_i d_i| of the rounded operands: f64[nq, n]."""
    return np.abs(to_f32(q_codes, dtype).astype(np.float64)) @ np.abs(to_f32(d_codes, dtype).astype(np.float64)).T


def tol(q_codes, d_codes, dtype):
    """dim_pad * 2^-22 * sum |q_i d_i|.  Derivation: the products of two half values are exact in fp32 or rounded once
    (relative 2^-24); a chain of dim_pad accumulations in fp32 precision, each rounded OR truncated (relative 2^-23 of a
    partial sum bounded by sum |q_i d_i|), adds at most dim_pad * 2^-23 * sum |q_i d_i|; the bound is twice that."""
    dim_pad = np.asarray(q_codes).shape[1]
    return dim_pad * 2.0 ** -22 * abs_scores(q_codes, d_codes, dtype)
