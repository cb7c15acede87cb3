"""The top-k merge (srx_merge_topk and its packed forms) restated in NumPy from the contract in include/sparse_rx.h.

Imports nothing from the product.  Holds
  merge      the merge of a batch, the engine's (doc, score, count) triple;
  dispatch   which kernels srx_merge_impl launches for (n_lists, k): the tree levels, the final kernel, the workspace;
  layouts    one logical input laid out in the forms the four entry points take, and the packed form of a result;
  makers     seeded inputs of the families the tests run (make_input), and the condition the `ties` family must meet;
  CASES      the shape table of tests/test_merge_cpu.py and tests/test_merge_gpu.py.

A logical input is the triple (doc i32[nq, L, k], score f32[nq, L, k], count i32[nq, L]): list l of query q has k slots.
Scores travel as bit patterns wherever they are copied or compared (NaN payloads and -0.0 survive that way).
"""
from collections import namedtuple

import numpy as np

KMAX = 1024                # SRX_MAX_K
MERGE_CAP = 4096           # candidates one workgroup of the block kernel takes
WAVE_KMAX, WAVE_CAP, WAVE_LISTS = 128, 1024, 256  # the wave kernel's limits
DOC_MAX = 2 ** 31 - 2      # the largest doc id (0x7FFFFFFF - doc must not be 0)
POISON = 0x5A5A5A5A        # what the tests pre-fill every output word with


# ---------------------------------------------------------------------------------------------------------------
# the merge
# ---------------------------------------------------------------------------------------------------------------
def merge(lists, k):
    """Per query: every entry r < min(max(count, 0), k) of every list whose score is > 0 (NaN, -0.0, 0 and negatives are
    not; +inf and denormals are), ranked by (score bits descending, doc ascending), cut at k, padded with doc -1 / score 0.
    Doc ids are taken as they are.  Returns (doc i32[nq, k], score f32[nq, k], count i32[nq])."""
    doc, score, count = lists
    nq, n_lists, kk = doc.shape
    assert kk == k and score.shape == doc.shape and count.shape == (nq, n_lists)
    out_doc = np.full((nq, k), -1, np.int32)
    out_bits = np.zeros((nq, k), np.uint32)
    out_count = np.zeros(nq, np.int32)
    r = np.arange(k, dtype=np.int64)[None, :]
    for q in range(nq):
        n = np.clip(count[q].astype(np.int64), 0, k)[:, None]
        with np.errstate(invalid="ignore"):
            used = (r < n) & (score[q] > 0)
        d = doc[q][used].astype(np.int64)
        b = score[q][used].view(np.uint32).astype(np.int64)
        order = np.lexsort((d, -b))[:k]
        m = order.size
        out_doc[q, :m] = d[order]
        out_bits[q, :m] = b[order]
        out_count[q] = m
    return out_doc, out_bits.view(np.float32), out_count


# ---------------------------------------------------------------------------------------------------------------
# the dispatch of srx_merge_impl
# ---------------------------------------------------------------------------------------------------------------
Dispatch = namedtuple("Dispatch", "fan levels final final_lists workspace_bytes")


def dispatch(n_lists, k, nq=1):
    """fan = 4096 // k lists per workgroup; while more lists than that remain, a tree level folds groups of `fan` lists into
    one unordered list each (`levels` = the group count of every level); the final pass over what is left is the wave
    kernel when k <= 128, lists * k <= 1024 and lists <= 256, else the block kernel.  The workspace is two ping-pong
    buffers sized for the first level."""
    assert 1 <= k <= KMAX and n_lists >= 1 and nq >= 0
    fan = MERGE_CAP // k
    levels, lists = [], n_lists
    while lists > fan:
        lists = (lists + fan - 1) // fan
        levels.append(lists)
    final = "wave" if k <= WAVE_KMAX and lists * k <= WAVE_CAP and lists <= WAVE_LISTS else "block"
    ws = 0
    if levels:
        g = levels[0]
        ws = 2 * (nq * g * k * 8 + nq * g * 4 + 256)
    return Dispatch(fan, tuple(levels), final, lists, ws)


def bucket(n_lists, k):
    """The name the shape table uses: 'wave', 'block', 'tree1+wave', 'tree2+block', ..."""
    d = dispatch(n_lists, k)
    return d.final if not d.levels else f"tree{len(d.levels)}+{d.final}"


# (n_lists, k, bucket, nq).  Derived by hand from the rule; a row that lands in another bucket is moved, the assert stays.
CASES = [
    (1, 1, "wave", 3), (1, 128, "wave", 4), (8, 128, "wave", 5), (16, 64, "wave", 9), (10, 100, "wave", 1),
    (256, 4, "wave", 3), (256, 1, "wave", 4),
    (1, 129, "block", 5), (9, 128, "block", 9), (17, 64, "block", 1), (11, 100, "block", 3), (257, 3, "block", 4),
    (1024, 1, "block", 5), (4096, 1, "block", 3), (1, 1024, "block", 9), (4, 1024, "block", 4), (40, 100, "block", 5),
    (31, 129, "block", 1), (3, 513, "block", 3), (4, 1000, "block", 9),
    (4097, 1, "tree1+wave", 5), (41, 100, "tree1+wave", 9),
    (5, 1024, "tree1+block", 4), (16, 1024, "tree1+block", 3), (32, 129, "tree1+block", 5), (5, 1000, "tree1+block", 1),
    (1601, 100, "tree2+wave", 3),
    (17, 1024, "tree2+block", 4),
    (65, 1024, "tree3+block", 3),  # the third level writes the buffer the first level wrote: the ping-pong wraps
]
# nq = 1003: a partly filled last workgroup of four waves (wave kernel), a grid of nq * groups (tree)
BIG_CASES = [(10, 100, "wave", 1003), (41, 100, "tree1+wave", 1003)]
FAMILIES = ("distinct", "ties", "all_equal", "dirty", "unordered")
BIG_FAMILIES = ("distinct", "ties", "dirty")


def case_families(n_lists, families=FAMILIES):
    """`ties` needs the boundary tie group to sit in two lists: not for a single list."""
    return tuple(f for f in families if not (f == "ties" and n_lists < 2))


def case_seed(n_lists, k, nq, family):
    return 1_000_003 * n_lists + 7919 * k + 31 * nq + 1000 * FAMILIES.index(family) + 5


# ---------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------
def to_plain(lists):
    """[nq][L][k] + counts [nq][L]: srx_merge_topk, gathered == 0."""
    doc, score, count = lists
    return np.ascontiguousarray(doc), np.ascontiguousarray(score), np.ascontiguousarray(count)


def to_gathered(lists):
    """[L][nq][k] + counts [L][nq]: srx_merge_topk, gathered == 1."""
    doc, score, count = lists
    return (np.ascontiguousarray(doc.transpose(1, 0, 2)), np.ascontiguousarray(score.transpose(1, 0, 2)),
            np.ascontiguousarray(count.T))


def to_packed(lists):
    """[L][nq][2k+1] int32, row = k doc ids, k score bit patterns, the count: the two packed entry points."""
    doc, score, count = lists
    nq, n_lists, k = doc.shape
    p = np.empty((n_lists, nq, 2 * k + 1), np.int32)
    p[:, :, :k] = doc.transpose(1, 0, 2)
    p[:, :, k:2 * k] = score.view(np.int32).transpose(1, 0, 2)
    p[:, :, 2 * k] = count.T
    return p


def packed_rows(triple):
    """A result triple as the rows [nq][2k+1] srx_merge_topk_packed_out writes."""
    doc, score, count = triple
    nq, k = doc.shape
    p = np.empty((nq, 2 * k + 1), np.int32)
    p[:, :k] = doc
    p[:, k:2 * k] = score.view(np.int32)
    p[:, 2 * k] = count
    return p


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------
def _unique_ints(rng, n, lo, hi):
    """n distinct integers of [lo, hi) in random order (hi - lo far larger than n)."""
    got = np.unique(rng.integers(lo, hi, size=n + n // 4 + 16, dtype=np.int64))
    while got.size < n:
        got = np.unique(np.concatenate([got, rng.integers(lo, hi, size=n + 16, dtype=np.int64)]))
    return rng.permutation(got)[:n]


def _unique_docs(rng, n):
    """n distinct doc ids of [0, DOC_MAX] in random order, both ends among them (one of them when n == 1)."""
    ids = _unique_ints(rng, n, 1, DOC_MAX)
    if n == 1:
        ids[0] = (0, DOC_MAX)[int(rng.integers(2))]
    else:
        a, b = rng.choice(n, 2, replace=False)
        ids[a], ids[b] = 0, DOC_MAX
    return ids


def _distinct_bits(rng, n):
    """n distinct positive normal fp32 bit patterns over the whole exponent range."""
    return _unique_ints(rng, n, 0x00800000, 0x7F000000)


def _order_lists(doc, bits, count):
    """Well-formed lists: the entries inside count ranked (score descending, doc ascending), the way a search writes them."""
    n_lists, k = doc.shape
    inside = np.arange(k)[None, :] < np.clip(count, 0, k)[:, None]
    key = np.where(inside, (bits << 31) | (0x7FFFFFFF - doc), -1)
    order = np.argsort(-key, axis=1, kind="stable")
    return np.take_along_axis(doc, order, 1), np.take_along_axis(bits, order, 1)


def _pad(doc, bits, count):
    k = doc.shape[1]
    outside = np.arange(k)[None, :] >= np.clip(count, 0, k)[:, None]
    doc[outside], bits[outside] = -1, 0


def _counts(rng, q, n_lists, k):
    """Per-list counts of 0 .. k, an empty and a full list among them; every second query holds fewer than k entries in all."""
    if q % 2 == 1:
        return rng.multinomial(int(rng.integers(0, k)), np.full(n_lists, 1.0 / n_lists)).astype(np.int64)
    c = rng.integers(0, k + 1, size=n_lists, dtype=np.int64)
    if n_lists >= 2:
        a, b = rng.choice(n_lists, 2, replace=False)
        c[a], c[b] = 0, k
    return c


# what `dirty` puts inside count: +0, -0.0, -1, -FLT_MAX, -inf, three NaNs -- none of them > 0 --, then +inf, the smallest
# positive denormal, FLT_MAX and the smallest normal, which are
_SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0xBF800000, 0xFF7FFFFF, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
                          0x7F800000, 0x00000001, 0x7F7FFFFF, 0x00800000, 0x7F800000, 0x00000001], np.int64)
_BIG_COUNTS = (1, 7, 2 ** 31 - 1)       # added to / replacing k
_NEG_COUNTS = (-1, -3, -2 ** 31)


def _query(rng, family, q, n_lists, k):
    n = n_lists * k
    doc = _unique_docs(rng, n).reshape(n_lists, k)
    if family == "all_equal":
        bits = np.full((n_lists, k), int(_distinct_bits(rng, 1)[0]), np.int64)
        count = np.full(n_lists, k, np.int64)
        doc, bits = _order_lists(doc, bits, count)
    elif family == "ties":
        # three values; n_hi < k entries of the best one, then more of the middle one than the k - n_hi that fit
        lo, mid, hi = np.sort(_distinct_bits(rng, 3))
        n_hi = int(rng.integers(0, k))
        n_mid = int(rng.integers(max(k - n_hi + 1, 2), n - n_hi + 1))
        flat = np.full(n, lo, np.int64)
        flat[:n_hi], flat[n_hi:n_hi + n_mid] = hi, mid
        bits = rng.permutation(flat).reshape(n_lists, k)
        # a member of the boundary group in the first and in the last list (the first and the last first-level group)
        for l in (0, n_lists - 1):
            if not (bits[l] == mid).any():
                have = (bits == mid).sum(axis=1)
                have[0] -= l != 0  # list 0 keeps one
                ls = int(np.argmax(have))
                rs = int(np.flatnonzero(bits[ls] == mid)[0])
                r = int(rng.integers(k))
                bits[l, r], bits[ls, rs] = mid, bits[l, r]
        count = np.full(n_lists, k, np.int64)
        doc, bits = _order_lists(doc, bits, count)
    elif family in ("distinct", "unordered"):
        bits = _distinct_bits(rng, n).reshape(n_lists, k)
        count = _counts(rng, q, n_lists, k)
        if family == "distinct":
            doc, bits = _order_lists(doc, bits, count)
        _pad(doc, bits, count)
    elif family == "dirty":
        bits = _distinct_bits(rng, n).reshape(n_lists, k)
        count = rng.integers(0, k + 1, size=n_lists, dtype=np.int64)
        kind = rng.integers(0, 4, size=n_lists)
        big, neg = kind == 0, kind == 1
        count[big] = np.minimum(k + rng.choice(_BIG_COUNTS, size=int(big.sum())), 2 ** 31 - 1)
        count[neg] = rng.choice(_NEG_COUNTS, size=int(neg.sum()))
        if q % 2 == 0:
            count[0] = -1  # the first list's count is negative: an empty list like any other
        inside = np.arange(k)[None, :] < np.clip(count, 0, k)[:, None]
        slots = np.flatnonzero(inside.reshape(-1))
        pick = rng.permutation(slots)[:min(len(_SPECIAL_BITS), len(slots))]
        bits.reshape(-1)[pick] = _SPECIAL_BITS[:len(pick)]
        # after count: large positive scores with ids of their own -- the best rows of the query, were they read
        bits[~inside] = rng.integers(0x7E000000, 0x7F000000, size=int((~inside).sum()), dtype=np.int64)
    else:
        raise ValueError(family)
    return doc, bits, count


def make_input(family, nq, n_lists, k, seed):
    """The logical input of one case.  No doc id twice in a query (every slot, padding and junk included, has an id of its
    own unless it is the -1 of clean padding); ids span 0 .. 2^31 - 2 with both ends present."""
    rng = np.random.default_rng(seed)
    doc = np.empty((nq, n_lists, k), np.int32)
    score = np.empty((nq, n_lists, k), np.uint32)
    count = np.empty((nq, n_lists), np.int32)
    for q in range(nq):
        d, b, c = _query(rng, family, q, n_lists, k)
        doc[q], score[q], count[q] = d, b, c
    return doc, score.view(np.float32), count


def tie_boundary_ok(lists, k, fan):
    """Per query: does the k-th boundary fall strictly inside a tie group (fewer than k entries above it, more than k with
    it) whose members sit in at least two lists -- in at least two first-level groups when the case has a tree?"""
    doc, score, count = lists
    nq, n_lists, _ = doc.shape
    ok = np.zeros(nq, bool)
    r = np.arange(k)[None, :]
    for q in range(nq):
        used = (r < np.clip(count[q].astype(np.int64), 0, k)[:, None]) & (score[q] > 0)
        b = score[q].view(np.uint32)
        ranked = np.sort(b[used])[::-1]
        if ranked.size <= k:
            continue
        t = ranked[k - 1]
        n_gt, n_ge = int((ranked > t).sum()), int((ranked >= t).sum())
        where = np.unique(np.nonzero(used & (b == t))[0])
        if n_lists > fan:
            where = np.unique(where // fan)
        ok[q] = n_gt < k < n_ge and where.size >= 2
    return ok
