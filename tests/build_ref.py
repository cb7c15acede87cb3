"""NumPy restatements of what the index-build entry points promise (include/sparse_rx.h): the checkers of
tests/test_build_cpu.py and tests/test_build_gpu.py.  float64 / integer arithmetic where it matters, one float32 rounding per
operation where the contract is a float32 expression.

  layout          the blocked layout, vectorised (5 M postings in about a second).  Written from the header's description, not
                  from the kernels' arithmetic; trusted on large inputs only because test_build_cpu.py asserts that it equals
                  parity.np_build_blocks (the loop form) bit for bit on every small directed case.
  compact         the compact copy (parity.np_compact_blocks).
  term_bounds     the K-th largest value of every term.
  sum_groups      left-to-right float32 sums of runs of duplicates.
  auto_unit_tiles the unit srx_auto_unit_tiles picks.
BM25 impacts are oracle.np_oracle.impacts_f32."""
import math

import numpy as np

from parity import np_compact_blocks

BLOCK_PAD = 256  # SRX_BLOCK_PAD
UNIT_MAX_DOCS = 49152  # docs of the largest unit that has a compact copy; the sentinels' compact ids start here
MAX_UNIT_TILES = 64
KMAX = 1024  # SRX_MAX_K: the largest rank srx_build_term_bounds takes
TERM_BOUND_GRID = 4096  # workgroups of srx_term_bounds_kernel at most: term t is served by workgroup t mod 4096
CAP_SKIP = 16384 * 256  # elements one trip of srx_tile_skip_kernel / srx_blocks_skip_kernel / srx_blocks_scatter_kernel covers
CAP_IMPACT = 8192 * 256  # ... of srx_impact_kernel / srx_sum_groups_kernel


def layout(rows, cols, vals, n_docs, vocab, tile_log2, unit_tiles, val_dtype=np.float32):
    """The blocked layout of srx_index_desc from COO triples with every (row, col) at most once (any order).
    Returns (term_ptr i64[V + 1], post i32[(n_blocks + 256) * words], tile_skip i32[V * (n_tiles + 1)], n_blocks), the tuple of
    parity.np_build_blocks.

    Postings are sorted by (term, doc).  A run is the postings of one term inside one unit of unit_tiles * G docs; every run,
    the empty ones included, is padded to a multiple of 4 with sentinels (doc -1 - 32 (t mod 64), value 0) and the runs follow
    each other in (term, unit) order.  tile_skip[t, j] = padded start of the run that tile j lies in, relative to the term's
    start, plus the postings of that run whose doc lies below j * G; tile_skip[t, n_tiles] = the term's padded length."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    with np.errstate(over="ignore"):
        vals = np.asarray(vals, np.float32).astype(val_dtype)
    V, G = int(vocab), 1 << tile_log2
    n_tiles = (n_docs + G - 1) >> tile_log2
    n_units = (n_tiles + unit_tiles - 1) // unit_tiles
    words = 8 if val_dtype == np.float32 else 6
    order = np.lexsort((rows, cols))
    t, d, v = cols[order], rows[order], vals[order]
    assert len(t) == 0 or (t[0] >= 0 and t[-1] < V and d.min() >= 0 and d.max() < n_docs)
    assert not np.any((t[1:] == t[:-1]) & (d[1:] == d[:-1])), "a (doc, term) pair twice: sum the duplicates first"
    run = t * n_units + d // (unit_tiles * G)
    run_len = np.bincount(run, minlength=V * n_units).astype(np.int64)
    real_start = np.concatenate([[0], np.cumsum(run_len)])  # position of a run's first posting among the real postings
    pad_start = np.concatenate([[0], np.cumsum((run_len + 3) // 4 * 4)])  # ... among the padded ones
    term_ptr = pad_start[np.arange(V + 1) * n_units].astype(np.int64)
    total = int(pad_start[-1])
    n_blocks = total // 4
    # every padded position starts as its term's sentinel, the real postings then take their places
    term_of_pos = np.repeat(np.arange(V, dtype=np.int64), np.diff(term_ptr))
    dd = np.concatenate([-1 - 32 * (term_of_pos % 64), np.repeat(-1 - 32 * (np.arange(BLOCK_PAD, dtype=np.int64) % 64), 4)])
    vv = np.zeros(total + 4 * BLOCK_PAD, val_dtype)
    pos = pad_start[run] + (np.arange(len(t), dtype=np.int64) - real_start[run])
    dd[pos] = d
    vv[pos] = v
    post = np.zeros((n_blocks + BLOCK_PAD, words), np.int32)
    post[:, :4] = dd.astype(np.int32).reshape(-1, 4)
    post[:, 4:] = vv.reshape(-1, 4).view(np.int32).reshape(n_blocks + BLOCK_PAD, -1)
    # postings of term t below tile edge j, then the same inside the run that tile j belongs to
    per_tile = np.bincount(t * n_tiles + (d >> tile_log2), minlength=V * n_tiles).reshape(V, n_tiles)
    below = np.zeros((V, n_tiles + 1), np.int64)
    np.cumsum(per_tile, axis=1, out=below[:, 1:])
    unit_of_tile = np.arange(n_tiles) // unit_tiles
    run_pad_start = pad_start[:-1].reshape(V, n_units) - term_ptr[:V, None]
    skip = np.empty((V, n_tiles + 1), np.int64)
    skip[:, :n_tiles] = run_pad_start[:, unit_of_tile] + (below[:, :n_tiles] - below[:, unit_of_tile * unit_tiles])
    skip[:, n_tiles] = np.diff(term_ptr)
    assert skip.max(initial=0) < 2 ** 31
    return term_ptr, post.reshape(-1), skip.astype(np.int32).reshape(-1), n_blocks


def compact(post, unit_docs, val_dtype=np.float32):
    """The compact copy of `post` (srx_build_compact)."""
    return np_compact_blocks(post, unit_docs, val_dtype)


def term_bounds(term_ptr, vals, ks):
    """srx_build_term_bounds: (out f32[V, len(ks)], neg_flag).  Per term the values, as float32, sorted descending; out[t, j] =
    element ks[j] - 1 where it exists and is > 0, else 0.  A NaN is not a value (it is never counted); neg_flag = some value
    is < 0 (-0.0 and NaN are not)."""
    term_ptr = np.asarray(term_ptr, np.int64)
    x = np.asarray(vals).astype(np.float32)
    ks = np.asarray(ks, np.int64)
    assert 1 <= len(ks) <= 64 and ks.min() >= 1 and ks.max() <= KMAX
    out = np.zeros((len(term_ptr) - 1, len(ks)), np.float32)
    for t in range(len(term_ptr) - 1):
        s = x[term_ptr[t]:term_ptr[t + 1]]
        s = np.sort(s[~np.isnan(s)])[::-1]
        have = ks <= len(s)
        e = s[np.where(have, ks - 1, 0)] if len(s) else np.zeros(len(ks), np.float32)
        out[t] = np.where(have & (e > 0), e, np.float32(0))
    return out, bool(np.any(x < 0))


def sum_groups(first, vals):
    """srx_build_sum_duplicates: out[g] = ((vals[a] + vals[a + 1]) + ...) + vals[b - 1] for [a, b) = first[g : g + 2], float32, one
    rounding per add."""
    first = np.asarray(first, np.int64)
    vals = np.asarray(vals, np.float32)
    a, n = first[:-1], np.diff(first)
    assert np.all(n >= 1)
    s = vals[a].copy()
    for i in range(1, int(n.max(initial=1))):
        m = n > i
        s[m] = s[m] + vals[a[m] + i]
    return s


def sum_groups_reversed(first, vals):
    """The same groups summed right to left: what the order-sensitivity check compares with."""
    first = np.asarray(first, np.int64)
    vals = np.asarray(vals, np.float32)
    e, n = first[1:] - 1, np.diff(first)
    s = vals[e].copy()
    for i in range(1, int(n.max(initial=1))):
        m = n > i
        s[m] = s[m] + vals[e[m] - i]
    return s


def auto_unit_tiles(n_docs, vocab, nnz, tile_log2):
    """srx_auto_unit_tiles as csrc/build.hip documents it: the largest unit of t tiles, t <= 64 and t * G <= 49152 docs, for which
    the run of an average term inside a unit -- mean = nnz / (n_docs * vocab) * t * G postings, taken as Poisson -- stays
    within the 8 x 12 register slots of its lane group at mean + 5 sigma; at least one tile.  Python floats are the doubles
    of the C function; the products are taken in its order."""
    assert n_docs > 0 and vocab > 0 and nnz >= 0 and 6 <= tile_log2 <= 14
    most = min(MAX_UNIT_TILES, UNIT_MAX_DOCS >> tile_log2)
    density = float(nnz) / (float(n_docs) * float(vocab))

    def fits(t):
        mean = density * float(t) * float(1 << tile_log2)
        return mean + 5.0 * math.sqrt(mean) <= 8.0 * 12

    t = 1
    while t < most and fits(t + 1):
        t += 1
    return t
