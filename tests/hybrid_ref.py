"""NumPy restatement of the hybrid fusion contract (include/sparse_rx.h), written from the
contract's text: a dict per query, ``np.float32`` scalars (every operation rounded to fp32 on its own, IEEE divide,
denormals kept), ``sorted`` by (-score, doc).  The GPU tests compare the kernel's rows with this bit for bit.

Also here: the host dispatch rule restated (which of the kernel's two forms a shape takes) and the seeded list maker
the kernel tests share."""
import functools

import numpy as np

WEIGHTED, RRF = 0, 1
MODES = {"weighted": WEIGHTED, "rrf": RRF}
MAX_K = 1024
WAVE_MAX_CANDIDATES, WAVE_MAX_K = 1024, 128


def form(ka: int, kb: int, k: int) -> str:
    """Which kernel form the host picks: one wavefront per query for small shapes, one workgroup otherwise."""
    return "wave" if ka + kb <= WAVE_MAX_CANDIDATES and k <= WAVE_MAX_K else "block"


# ---- the kernels' open-addressing table restated (csrc/fuse.hip: fuse_slot, fuse_insert, fuse_find) -----------------------------
F_SLOTS, F_SLOT_BITS, F_MULTIPLIER = 2048, 11, 2654435761
MAX_DOC = 2 ** 31 - 2  # the largest doc id the engine's ranking key (0x7FFFFFFF - doc, 0 = none) can carry


def fuse_slot(doc):
    """home slot of a doc id >= 0: the top F_SLOT_BITS bits of (doc * F_MULTIPLIER mod 2^32)"""
    return (((np.asarray(doc, np.int64) * F_MULTIPLIER) & 0xFFFFFFFF) >> (32 - F_SLOT_BITS)).astype(np.int64)


@functools.lru_cache(maxsize=4)
def _homes(lo, hi):
    ids = np.arange(lo, hi, dtype=np.int64)
    return ids, fuse_slot(ids).astype(np.int16)


def docs_homed_at(slots, n, lo, hi):
    """the n smallest doc ids of [lo, hi) whose home slot is `slots` (one slot) or one of `slots`, ascending, int32"""
    ids, home = _homes(lo, hi)
    pick = ids[home == slots] if np.isscalar(slots) else ids[np.isin(home, np.asarray(list(slots), np.int64))]
    assert len(pick) >= n, (slots, n, lo, hi, len(pick))
    return pick[:n].astype(np.int32)


def probe_layout(docs):
    """int64[F_SLOTS]: the doc each slot holds (-1 = empty) after the docs are entered by linear probing with wrap.  Which
    doc lands where depends on the order of insertion; WHICH SLOTS are occupied does not."""
    tbl = np.full(F_SLOTS, -1, np.int64)
    assert len(docs) < F_SLOTS
    for d, h in zip(np.asarray(docs).tolist(), fuse_slot(docs).tolist()):
        while tbl[h] >= 0:
            h = (h + 1) & (F_SLOTS - 1)
        tbl[h] = d
    return tbl


def probe_walk(tbl, doc):
    """(found, slots visited in order) of fuse_find's walk for `doc`: from its home slot to its own slot or the first empty one"""
    h = int(fuse_slot(doc))
    seen = []
    for _ in range(F_SLOTS):
        seen.append(h)
        if tbl[h] < 0:
            return False, seen
        if tbl[h] == doc:
            return True, seen
        h = (h + 1) & (F_SLOTS - 1)
    return False, seen


def _used(doc, score, count, kx):
    """positions of the used entries of one list row: r < min(max(count, 0), kx), doc >= 0, score > 0"""
    n = min(max(int(count), 0), kx)
    return [r for r in range(n) if doc[r] >= 0 and score[r] > 0]


def _contributions(doc, score, count, w, mode, rrf_c):
    kx = len(doc)
    used = _used(doc, score, count, kx)
    w = np.float32(w)
    out = {}
    if mode == WEIGHTED:
        if 0 not in used:  # the list's head is not used: the list counts as empty in this mode
            return out
        m = np.float32(score[0])
        for r in used:
            out[int(doc[r])] = np.float32(w * np.float32(np.float32(score[r]) / m))
    else:
        c = np.float32(rrf_c)
        for r in used:
            out[int(doc[r])] = np.float32(w / np.float32(c + np.float32(r + 1)))
    return out


def fuse_row(a_doc, a_score, a_count, b_doc, b_score, b_count, k, mode, wa, wb, rrf_c=60.0):
    """One query: ranked [(doc, fused score f32)], at most k entries, fused score > 0 only."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ca = _contributions(a_doc, a_score, a_count, wa, mode, rrf_c)
        cb = _contributions(b_doc, b_score, b_count, wb, mode, rrf_c)
        fused = dict(ca)
        for d, c in cb.items():
            fused[d] = np.float32(fused[d] + c) if d in fused else c
    rows = [(d, s) for d, s in fused.items() if s > 0]
    rows.sort(key=lambda t: (-int(np.float32(t[1]).view(np.uint32)), t[0]))  # positive floats: bit order = value order
    return rows[:k]


def fuse(a, b, k, mode="weighted", weights=(0.3, 0.7), rrf_c=60.0):
    """Batch form with the engine's output layout: (doc i32[nq, k], score f32[nq, k], count i32[nq]), padded -1 / 0."""
    (a_doc, a_score, a_count), (b_doc, b_score, b_count) = a, b
    code = MODES[mode] if isinstance(mode, str) else mode
    nq = len(a_count)
    doc = np.full((nq, k), -1, np.int32)
    score = np.zeros((nq, k), np.float32)
    count = np.zeros(nq, np.int32)
    for q in range(nq):
        rows = fuse_row(a_doc[q], a_score[q], a_count[q], b_doc[q], b_score[q], b_count[q], k, code, weights[0], weights[1], rrf_c)
        count[q] = len(rows)
        for r, (d, s) in enumerate(rows):
            doc[q, r], score[q, r] = d, s
    return doc, score, count


def make_lists(rng, nq, ka, kb, overlap=0.5, n_docs=1 << 20, score_range=(0.5, 30.0), fill=(0.3, 1.0), garbage=True):
    """Two seeded list batches in the engines' form: per query a random count (``fill`` = fraction range of kx; at least
    one query of a batch of >= 2 gets the full row), descending positive scores, unique docs inside a list, padding
    -1 / 0 -- or, with ``garbage``, plausible-looking junk beyond ``count`` that must be ignored.  ``overlap`` = the
    fraction of list B's docs drawn from list A's."""
    def one_side(kx, pool_fn):
        doc = np.full((nq, kx), -1, np.int32)
        score = np.zeros((nq, kx), np.float32)
        count = np.zeros(nq, np.int32)
        for q in range(nq):
            n = kx if (q == nq - 1 and nq >= 2) else int(np.clip(round(kx * rng.uniform(*fill)), 0, kx))
            docs = pool_fn(q, n)
            n = len(docs)
            lo, hi = score_range
            s = np.sort(np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.float32))[::-1]
            doc[q, :n], score[q, :n], count[q] = docs, s, n
            if garbage and n < kx:
                doc[q, n:] = rng.integers(0, n_docs, kx - n)
                score[q, n:] = rng.uniform(1.0, 100.0, kx - n).astype(np.float32)
        return doc, score, count

    a = one_side(ka, lambda q, n: rng.choice(n_docs, n, replace=False).astype(np.int32))

    def b_pool(q, n):
        a_docs = a[0][q, : a[2][q]]
        n_common = min(int(round(n * overlap)), len(a_docs))
        common = rng.choice(a_docs, n_common, replace=False) if n_common else np.zeros(0, np.int32)
        fresh = []
        taken = set(a_docs.tolist())
        while len(fresh) < n - n_common:
            d = int(rng.integers(0, n_docs))
            if d not in taken:
                taken.add(d)
                fresh.append(d)
        docs = np.concatenate([common.astype(np.int32), np.array(fresh, np.int32)])
        return docs[rng.permutation(len(docs))]

    b = one_side(kb, b_pool)
    return a, b
