"""The sparse family at scale, as a table: one row per index whose posting blocks, padded positions or skip-table entries lie
on both sides of a 32-bit boundary of the address arithmetic.  A plain module, as dense_scale.py is: it never imports the
package.  tests/test_sparse_scale_cpu.py proves the arithmetic of every row with Python integers and builds every row a second
time with its boundaries scaled down, where the whole index is small enough to be compared word for word with
parity.np_build_blocks; tests/test_sparse_scale_gpu.py runs the rows and nothing else.

Construction: the index of a case is one zero-filled device arena.  Only the PLANTED terms hold data:
their blocks, their rows of tile_skip, their idf and term_bound entries.  Every other term is a FILLER term: it owns an extent
of the posting array (that is what pushes the planted terms to the wanted positions) or nothing at all (that is what pushes
them to the wanted term ids), and no query of the case names it.  The kernels read the posting extent and the skip row of a
query's terms only, so the expected rows are the oracle's on the planted postings alone: O(planted) on the host.

Boundaries, in the units the kernels multiply: a block index times the block width crosses 2^31 / 2^32 BYTES of post / post16
and 2^31 32-bit WORDS of them; a padded position term_ptr + skip crosses 2^31 / 2^32; t * (n_tiles + 1) + j crosses the 2^30
entries of tier1_cannot_serve's clause and 2^31.

Planted terms come in GROUPS of consecutive terms that are contiguous in the posting array.  A group placed at a boundary has
one run (the postings of one term inside one unit) whose middle block is the block that holds -- or starts at -- the boundary:
the group's terms before that run end below it, the terms behind it start above it.  The posting shapes are the directed
ones of test_tier1_routes_cpu.py and test_tier2_routes_cpu.py:
  A  case_a(4): a long term with runs of 4 LPT, 4 LPT + 1, 8 LPT, 8 LPT + 1, 12 LPT (served by tier 1 with one, two and three
     blocks per lane) and 12 LPT + 1 postings (flagged) in units 0 .. 5, LPT = 16, and three short terms, the last of which
     also has the shard's third-last doc (so a group that ends the vocabulary reads the very last entry of the skip table);
     queried with all four terms, with the long term alone and with the last term alone;
  B  case_b("two"): two terms whose units need 0, 48 (served), 49 (flagged), 1 and 0 multi-term resolutions, and a short term;
  H  case_d3(12): two terms with 2048 + 2048 postings in unit 5 (P = 4096: tier 2's hash unit) and 2048 + 2049 in unit 6
     (P = 4100: a dense tile, served by the wave-level dense path; the packed path under SRX_DBG_NO_WAVE_DENSE), a short term;
  E  one short term with postings in the first unit and on the last two docs of the shard: term 0 and the last term.
Every unit is 4096 docs: tile_log2 12 with one-tile units, or tile_log2 6 with 64-tile units (1025 skip entries per term)."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import parity
from dense_scale import CAP_BYTES, GARBAGE, GUARD_WORDS, MAX_ID, r256  # noqa: F401  (the GPU test reads them from here)

F = np.float32
BLOCK_PAD = 256   # SRX_BLOCK_PAD
U = 4096          # docs per unit, in every case
K = 10            # top-k of every search of the table
LOW = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0)                      # test_tier1_routes_cpu.LOW
B_VALUES = (0.125, 0.5, 1.0, 3.0, 7.0, 12.5, 0.25, 40.0)   # test_tier1_routes_cpu.B_VALUES
BLOCK_WORDS = {("f32", "post"): 8, ("f16", "post"): 6, ("f32", "post16"): 6, ("f16", "post16"): 4}
VAL_DTYPE = {"f32": np.float32, "f16": np.float16}
VAL_TYPE = {"f32": 0, "f16": 1}  # srx_val_type


def _f16_ramp(n, start=0x3C00):
    return np.arange(start, start + n, dtype=np.uint16).view(np.float16).astype(np.float32)


# ---- the groups: (postings (doc, local term, value), idf per local term, queries [(local terms, weights)], straddle term) -------
def _group_a(g, n_docs):
    """local terms 0, 2, 3: the short ones; 1: the long one"""
    L = 16
    runs = [4 * L, 4 * L + 1, 8 * L, 8 * L + 1, 12 * L, 12 * L + 1, 0, 0]
    base, off, others = 12 * L + 3, 5 * g, (0, 2, 3)
    posts = []
    for u, run in enumerate(runs):
        for i in range(run):
            v = LOW[(i + u + g) % len(LOW)]
            if i >= run - 2:
                v = 30.0 - 2 * u - (i - (run - 2))
            posts.append((u * U + off + i, 1, v))
        if u != 6:
            for j, t in enumerate(others):
                for r in range(1 + (j + u) % 3):
                    posts.append((u * U + off + base + 3 * j + r, t, LOW[(j + r + u + g) % len(LOW)]))
    posts.append((n_docs - 3, 3, 12.5))  # the group's last term ends in the shard's last unit: its run there ends at skip[n_tiles]
    idf = [0.3, 2.0 + g / 8, 0.31, 0.32]
    return posts, idf, [((0, 1, 2, 3), (0.25, 1.5, 0.5, 0.75)), ((1,), (1.5,)), ((3,), (1.0,))], 1


def _group_b(g, n_docs):
    """local term 0: the short one; 1, 2: case_b("two")'s pair"""
    units = [[(0,)] * 5 + [(1,)] * 6, [(0, 1)] * 48 + [(0,)] * 3, [(0, 1)] * 49 + [(1,)] * 2, [(0, 1)] + [(0,), (1,)] * 4, [(1,)] * 3]
    posts, n = [(3 + g, 0, 1.0), (9 + g, 0, 2.0), (7 * U + 5 + g, 0, 0.5)], 0
    for u, docs in enumerate(units):
        off = (0, 31, 17, 64, 5)[u] + g
        for i, slots in enumerate(docs):
            for s in slots:
                posts.append((u * U + off + i, 1 + s, B_VALUES[(n + s + g) % len(B_VALUES)]))
                n += 1
    idf = [0.4, 0.05 * 1.7 ** (g % 9), 0.05 * 1.7 ** ((g + 1) % 9)]
    w = (2.0 ** -3 * 1.0, 2.0 ** -2 * 1.1)
    return posts, idf, [((1, 2), w), ((2, 1), w[::-1]), ((0,), (1.0,))], 1


def _group_h(g, n_docs):
    """local term 0: the short one; 1, 2: case_d3's pair.  Values ascend along the rotated doc order of a unit."""
    ramp = _f16_ramp(9000)
    posts = [(100 + g, 0, 1.0), (U + 7 + g, 0, 3.0), (2 * U + g, 0, 0.75)]
    for i in range(4096):
        d = 5 * U + (i + 7 * g) % U
        posts.append((d, 1, ramp[2 * i]) if i < 2048 else (d, 2, ramp[4096 + 2 * (i - 2048)]))
    for i in range(4096):
        d = 6 * U + (i + 7 * g) % U
        if i < 2048:
            posts.append((d, 1, ramp[2 * i + 1]))
        if i >= 2047:
            posts.append((d, 2, ramp[4097 + 2 * (i - 2047)]))
    return posts, [0.7, 1.0 + g / 16, 1.0], [((1, 2), (1.0, 1.0)), ((0,), (2.0,))], 1


def _group_e(g, n_docs):
    posts = [(g, 0, 1.5), (g + 1, 0, 0.75), (g + 40, 0, 3.0), (n_docs - 2, 0, 2.0), (n_docs - 1, 0, 1.0)]
    return posts, [0.9 + g / 32], [((0,), (1.0,))], 0


GROUPS = {"A": _group_a, "B": _group_b, "H": _group_h, "E": _group_e}


@dataclass(frozen=True)
class Case:
    name: str
    val: str            # "f32" | "f16": the stored value type
    copies: tuple       # which of "post" (canonical) and "post16" (compact) the descriptor carries
    tile_log2: int
    unit_tiles: int
    n_units: int
    groups: tuple       # ((kind, straddle unit of the straddle term, place), ...) in array order
    shrink: int         # the scaled-down build: every boundary exponent minus this
    vocab_rule: tuple = ()  # () = the last planted term ends the vocabulary; ("lt", e) / ("ge", e): vocab * (n_tiles + 1) is the
    #                         largest product below / the first at or above 2^e, and the last group ends the vocabulary
    note: str = ""

    # places: ("start",) position 0, term 0; ("next",) right behind the previous group; ("bytes", copy, e) / ("words", copy, e):
    # byte / 32-bit word 2^e of that copy; ("pos", e): padded position 2^e; ("entry", e): the straddle term's skip row holds
    # entry 2^e of the table; ("end",): the group's last term is term vocab - 1
    @property
    def n_docs(self):
        return self.n_units * U - 3

    @property
    def n_tiles(self):
        return (self.n_docs + (1 << self.tile_log2) - 1) >> self.tile_log2

    @property
    def row(self):
        return self.n_tiles + 1

    @property
    def doc_base_top(self):
        return MAX_ID - self.n_docs

    def words(self, copy):
        return BLOCK_WORDS[(self.val, copy)]

    def boundary_block(self, place, shrink=0):
        """the block that holds (or starts at) the boundary of a posting place"""
        kind = place[0]
        if kind == "bytes":
            return (1 << (place[2] - shrink)) // (4 * self.words(place[1]))
        if kind == "words":
            return (1 << (place[2] - shrink)) // self.words(place[1])
        assert kind == "pos"
        return (1 << (place[1] - shrink)) // 4

    def filler_cap(self):
        """padded postings a filler term can really hold: a multiple of 4 per unit, so that its runs need no sentinel"""
        return sum(min(U, self.n_docs - u * U) // 4 * 4 for u in range(self.n_units))


@dataclass
class Layout:
    case: Case
    shrink: int
    vocab: int
    n_blocks: int
    term_ptr: np.ndarray     # i64[vocab + 1]
    planted: list            # per planted term: dict(term, small, group, ptr, extent)
    gaps: list               # per group: dict(first filler term, filler extents i64[n]) of the fillers in front of it
    places: list             # per group: dict(place, block or entry, term, unit) of the boundary it was placed at (None: no boundary)
    small: tuple             # (term_ptr, post i32[blocks + pad, words] with the big terms' sentinels, skip i32[P, row], n_blocks)
    csr: tuple               # the planted postings doc-major over the SMALL term ids: (indptr, indices, data)
    idf_small: np.ndarray
    queries_small: tuple     # (q_ptr, q_term, q_weight) over the small ids
    queries: tuple           # ... over the real ids

    def device_bytes(self):
        c = self.case
        n = sum((self.n_blocks + BLOCK_PAD) * c.words(cp) * 4 for cp in c.copies)
        n += self.vocab * c.row * 4 + (self.vocab + 1) * 8 + self.vocab * 4 + self.vocab * 16
        return n + (1 << 20)  # the workspace with its guard, the filter rows and the query batch: far below 1 MiB

    def posting_bytes(self, copy):
        return (self.n_blocks + BLOCK_PAD) * self.case.words(copy) * 4

    def term_bound(self):
        """f32[P, 4] of the planted terms (parity.BOUND_KS), from the stored values"""
        indptr, indices, data = self.csr
        out = np.zeros((len(self.planted), 4), F)
        for s in range(len(self.planted)):
            v = np.sort(data[indices == s])[::-1]
            for j, kk in enumerate(parity.BOUND_KS):
                if len(v) >= kk and v[kk - 1] > 0:
                    out[s, j] = v[kk - 1]
        return out

    def blocks_of(self, s, copy="post"):
        """the stored blocks of planted term s in one copy: i32[extent / 4, words]"""
        tp, post, _, _ = self.small
        b = post[tp[s] // 4: tp[s + 1] // 4]
        if copy == "post":
            return b
        return parity.np_compact_blocks(b.reshape(-1), U, VAL_DTYPE[self.case.val]).reshape(len(b), -1)

    def pad_blocks(self, copy="post"):
        tp, post, _, nb = self.small
        b = post[nb:]
        if copy == "post":
            return b
        return parity.np_compact_blocks(b.reshape(-1), U, VAL_DTYPE[self.case.val]).reshape(len(b), -1)

    def skip_row(self, s):
        return self.small[2][s]


def _batch(queries):
    q_ptr = np.zeros(len(queries) + 1, np.int32)
    q_ptr[1:] = np.cumsum([len(t) for t, _ in queries])
    q_term = np.concatenate([np.asarray(t, np.int32) for t, _ in queries])
    q_w = np.concatenate([np.asarray(w, np.float32) for _, w in queries])
    return q_ptr, q_term, q_w


@lru_cache(maxsize=None)
def build(case, shrink=0):
    """The layout of a case with every boundary exponent lowered by `shrink` (0: the case itself)."""
    c = case
    n_docs, dt = c.n_docs, VAL_DTYPE[c.val]
    # the planted postings over small term ids, group after group
    posts, idf, queries, first_small, straddle = [], [], [], [], []
    for g, (kind, su, place) in enumerate(c.groups):
        p, gi, gq, st = GROUPS[kind](g, n_docs)
        a = len(idf)
        first_small.append(a)
        posts += [(d, a + t, v) for d, t, v in p]
        idf += gi
        queries += [([a + t for t in ts], ws) for ts, ws in gq]
        straddle.append(a + st)
    P = len(idf)
    first_small.append(P)
    arr = np.array(sorted((int(d), int(t), float(v)) for d, t, v in posts), np.float64)
    docs, terms, vals = arr[:, 0].astype(np.int64), arr[:, 1].astype(np.int32), arr[:, 2].astype(np.float32)
    assert len(set(zip(docs.tolist(), terms.tolist()))) == len(docs) and 0 <= docs.min() and docs.max() < n_docs
    assert np.array_equal(vals.astype(np.float16).astype(np.float32), vals), "planted values must be fp16-exact"
    indptr = np.zeros(n_docs + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(docs, minlength=n_docs))
    tp, post, skip, nb = parity.np_build_blocks(indptr, terms, vals, n_docs, P, c.tile_log2, c.unit_tiles, dt, BLOCK_PAD)
    post = post.reshape(nb + BLOCK_PAD, -1).copy()
    skip = skip.reshape(P, c.row)
    # where the groups go
    cap = c.filler_cap()
    E = None
    if c.vocab_rule:
        E = 1 << (c.vocab_rule[1] - shrink)
        vocab_fixed = (E - 1) // c.row if c.vocab_rule[0] == "lt" else -(-E // c.row)
    pos, last_term = 0, -1  # the padded position behind the previous group, its last term
    starts, firsts, gaps, places = [], [], [], []
    for g, (kind, su, place) in enumerate(c.groups):
        a, b, S = first_small[g], first_small[g + 1], straddle[g]
        info = None
        if place[0] == "start":
            assert g == 0
            start, first = 0, 0
        elif place[0] == "next":
            start, first = pos, last_term + 1
        elif place[0] in ("bytes", "words", "pos"):
            run_lo = int(tp[S] + skip[S, su * c.unit_tiles])
            run_len = int(skip[S, min((su + 1) * c.unit_tiles, c.n_tiles)] - skip[S, su * c.unit_tiles])
            assert run_len >= 8 and run_len % 4 == 0, "the straddle run has blocks on both sides of its middle"
            bB = c.boundary_block(place, shrink)
            start = 4 * bB - (run_lo + 4 * (run_len // 8) - int(tp[a]))
            assert start >= pos, f"{c.name}: group {g} would overlap the one before it ({start} < {pos})"
            first = last_term + 1 + -(-(start - pos) // cap)
            info = {"place": place, "block": bB, "small": S, "unit": su, "run_blocks": run_len // 4}
        elif place[0] == "entry":
            e = 1 << (place[1] - shrink)
            start, first = pos, e // c.row - (S - a)
            assert first > last_term
            info = {"place": place, "entry": e, "small": S}
        else:
            assert place[0] == "end" and g == len(c.groups) - 1 and c.vocab_rule
            start, first = pos, vocab_fixed - (b - a)
            assert first > last_term
        n_fill = first - last_term - 1
        ext = np.zeros(n_fill, np.int64)
        gap = start - pos
        if gap:
            ext[:] = cap
            ext[-1] = gap - cap * (n_fill - 1)
            assert 0 < ext[-1] <= cap and ext[-1] % 4 == 0
        gaps.append({"first": last_term + 1, "extents": ext})
        starts.append(start)
        firsts.append(first)
        places.append(info)
        pos = start + int(tp[b] - tp[a])
        last_term = first + (b - a) - 1
    vocab = vocab_fixed if c.vocab_rule else last_term + 1
    assert vocab == last_term + 1
    extents = np.zeros(vocab, np.int64)
    planted = []
    for g in range(len(c.groups)):
        a, b = first_small[g], first_small[g + 1]
        extents[gaps[g]["first"]: gaps[g]["first"] + len(gaps[g]["extents"])] = gaps[g]["extents"]
        for s in range(a, b):
            t = firsts[g] + (s - a)
            extents[t] = tp[s + 1] - tp[s]
            planted.append({"term": t, "small": s, "group": g, "ptr": starts[g] + int(tp[s] - tp[a]), "extent": int(tp[s + 1] - tp[s])})
            rows = post[tp[s] // 4: tp[s + 1] // 4]  # the sentinels of the run padding carry the REAL term id
            rows[:, :4] = np.where(rows[:, :4] < 0, -1 - 32 * (t % 64), rows[:, :4])
    term_ptr = np.zeros(vocab + 1, np.int64)
    np.cumsum(extents, out=term_ptr[1:])
    assert all(term_ptr[p["term"]] == p["ptr"] for p in planted) and term_ptr[-1] == pos and pos % 4 == 0
    big = np.array([p["term"] for p in planted], np.int64)
    qs = _batch(queries)
    qb = (qs[0], big[qs[1]].astype(np.int32), qs[2])
    return Layout(c, shrink, vocab, pos // 4, term_ptr, planted, gaps, places, (tp, post, skip, nb), (indptr, terms, vals),
                  np.asarray(idf, F), qs, qb)


# ---- a whole index on the host: the scaled-down builds only -----------------------------------------------------------------------
def _filler_docs(case, extent):
    out, rem = [], int(extent)
    for u in range(case.n_units):
        n = min(rem, min(U, case.n_docs - u * U) // 4 * 4)
        out.append(u * U + np.arange(n, dtype=np.int64))
        rem -= n
    assert rem == 0
    return np.concatenate(out)


def materialize(lay):
    """(post i32[(n_blocks + pad), words], tile_skip i32[vocab, row], idf f32[vocab]) with the filler extents holding real filler
    postings: extent postings of value 1 on the first docs of unit after unit (a multiple of 4 per unit), in closed form."""
    c = lay.case
    words = c.words("post")
    tp_s, post_s, skip_s, nb_s = lay.small
    post = np.zeros((lay.n_blocks + BLOCK_PAD, words), np.int32)
    skip = np.zeros((lay.vocab, c.row), np.int32)
    idf = np.full(lay.vocab, 0.5, F)
    for p in lay.planted:
        post[p["ptr"] // 4: (p["ptr"] + p["extent"]) // 4] = lay.blocks_of(p["small"])
        skip[p["term"]] = skip_s[p["small"]]
        idf[p["term"]] = lay.idf_small[p["small"]]
    post[lay.n_blocks:] = lay.pad_blocks()
    one = np.ones(4, VAL_DTYPE[c.val]).view(np.int32)
    edges = np.arange(c.row, dtype=np.int64) << c.tile_log2
    for gap in lay.gaps:
        for i, e in enumerate(gap["extents"]):
            t = gap["first"] + i
            d = _filler_docs(c, e)
            b = post[lay.term_ptr[t] // 4: lay.term_ptr[t + 1] // 4]
            b[:, :4] = d.reshape(-1, 4)
            b[:, 4:] = one
            skip[t] = np.searchsorted(d, edges)
            skip[t, c.n_tiles] = e
    return post, skip, idf


def full_csr(lay):
    """the doc-major CSR (indptr, indices over the REAL term ids, data) of the scaled-down index, filler postings included"""
    c = lay.case
    indptr, indices, data = lay.csr
    big = np.array([p["term"] for p in lay.planted], np.int64)
    docs = [np.repeat(np.arange(c.n_docs), np.diff(indptr))]
    terms, vals = [big[indices]], [data]
    for gap in lay.gaps:
        for i, e in enumerate(gap["extents"]):
            d = _filler_docs(c, e)
            docs.append(d)
            terms.append(np.full(len(d), gap["first"] + i, np.int64))
            vals.append(np.ones(len(d), F))
    docs, terms, vals = np.concatenate(docs), np.concatenate(terms), np.concatenate(vals)
    order = np.lexsort((terms, docs))
    ip = np.zeros(c.n_docs + 1, np.int64)
    ip[1:] = np.cumsum(np.bincount(docs, minlength=c.n_docs))
    return ip, terms[order].astype(np.int32), vals[order].astype(F)


# ---- expected results ----------------------------------------------------------------------------------------------------------------
def full_scores(csr, idf, q, n_docs):
    """f32[nq, n_docs]: the oracle's scores with the contributions added in the query's term order (dot mode: the stored value
    is the CSR entry)"""
    import oracle
    q_ptr, q_term, q_w = q
    out = np.zeros((len(q_ptr) - 1, n_docs), F)
    for i in range(len(q_ptr) - 1):
        lo, hi = int(q_ptr[i]), int(q_ptr[i + 1])
        out[i] = oracle.scores_given_order(*csr, None, idf, q_term[lo:hi], q_w[lo:hi], tfidf=True)
    return out


def ranked_rows(full, k, doc_base, allow=None, after=None):
    """The searches' contract from full score vectors: score > 0 only, (score desc, doc asc), ids = doc_base + row, padded
    -1 / +0.  allow: None or per query None / bool[n_docs]; after: None or (global doc i32[nq], score f32[nq])."""
    nq, n = full.shape
    od, os_, oc = np.full((nq, k), -1, np.int32), np.zeros((nq, k), F), np.zeros(nq, np.int32)
    for q in range(nq):
        s = full[q]
        ok = s > 0
        if allow is not None and allow[q] is not None:
            ok &= np.asarray(allow[q], bool)
        if after is not None:
            ad, as_ = int(after[0][q]), F(after[1][q])
            ok &= (s < as_) | ((s == as_) & (np.arange(n) + doc_base > ad))
        c = np.flatnonzero(ok)
        c = c[np.lexsort((c, -s[c].astype(np.float64)))][:k]
        od[q, :len(c)], os_[q, :len(c)], oc[q] = c + doc_base, s[c], len(c)
    return od, os_, oc


def tier1_serves(lay):
    """what tier1_cannot_serve says of every query of the case (nt <= 64 and k <= 112 everywhere in the table)"""
    c = lay.case
    return not parity.tier1_cannot_serve(1, K, c.unit_tiles, c.tile_log2, lay.vocab, c.n_tiles, 0, post16="post16" in c.copies)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
_POST = dict(tile_log2=12, unit_tiles=1, n_units=8, shrink=12)
_SKIP = dict(tile_log2=6, unit_tiles=64, n_units=16, shrink=14)
CASES = [
    # f32, both copies, 10.7 + 8.0 GiB: bytes 2^31 and 2^32 and word 2^31 of the canonical blocks AND of the compact copy
    Case("p-f32-both", "f32", ("post", "post16"), groups=(
        ("E", 0, ("start",)), ("A", 4, ("bytes", "post", 31)), ("H", 5, ("bytes", "post16", 31)), ("B", 1, ("bytes", "post", 32)),
        ("A", 2, ("bytes", "post16", 32)), ("H", 6, ("words", "post", 31)), ("A", 0, ("words", "post16", 31)), ("E", 0, ("next",))), **_POST),
    # f32, canonical blocks alone (every query is tier 2's), 16 GiB: padded position 2^31
    Case("p-f32-canonical", "f32", ("post",), groups=(
        ("E", 0, ("start",)), ("A", 4, ("bytes", "post", 31)), ("B", 1, ("bytes", "post", 32)), ("H", 5, ("words", "post", 31)),
        ("A", 2, ("pos", 31)), ("H", 6, ("next",)), ("E", 0, ("next",))), **_POST),
    # f16, the compact copy alone (post == NULL: tier 2 reads it too), 16 GiB: padded positions 2^31 and 2^32
    Case("p-f16-compact", "f16", ("post16",), groups=(
        ("E", 0, ("start",)), ("A", 0, ("bytes", "post16", 31)), ("B", 1, ("bytes", "post16", 32)), ("H", 6, ("pos", 31)),
        ("A", 4, ("pos", 32)), ("H", 5, ("next",)), ("E", 0, ("next",))), **_POST,
        note="word 2^31 of the compact f16 copy (4 words per block) IS padded position 2^31"),
    # f16, both copies, 8.0 + 5.3 GiB: the 6-word canonical blocks
    Case("p-f16-both", "f16", ("post", "post16"), groups=(
        ("E", 0, ("start",)), ("A", 2, ("bytes", "post", 31)), ("H", 5, ("bytes", "post16", 31)), ("B", 1, ("bytes", "post", 32)),
        ("A", 4, ("bytes", "post16", 32)), ("H", 6, ("words", "post", 31)), ("E", 0, ("next",))), **_POST),
    # the skip table: 1025 entries per term.  vocab * 1025 = 2^30 - 1024: tier 1 serves, the last term's row ends 4 KiB under byte 2^32
    Case("s-lt30", "f32", ("post", "post16"), groups=(("E", 0, ("start",)), ("B", 1, ("next",)), ("H", 5, ("next",)), ("A", 4, ("end",))),
         vocab_rule=("lt", 30), **_SKIP),
    # vocab * 1025 = 2^30 + 1: every query is tier 2's
    Case("s-ge30", "f32", ("post", "post16"), groups=(("E", 0, ("start",)), ("B", 1, ("next",)), ("H", 5, ("next",)), ("A", 4, ("end",))),
         vocab_rule=("ge", 30), **_SKIP),
    # more than 2^31 entries (8.0 GiB): t * 1025 + j passes int32 inside the long term's row
    Case("s-gt31", "f32", ("post", "post16"), groups=(("E", 0, ("start",)), ("H", 5, ("next",)), ("A", 4, ("entry", 31)), ("B", 1, ("next",)),
                                                       ("E", 0, ("next",))), **_SKIP),
]

# What no case reaches, with the byte count that shows it (the cap is dense_scale.CAP_BYTES = 24 GiB):
OUT_OF_REACH = {
    "block index 2^32 (the high half of tblk, wave_kernel.hip)": (1 << 32) * 16,         # 64 GiB of the smallest blocks (compact f16)
    "padded position 2^32 in canonical blocks": (1 << 30) * 24,                          # 24 GiB of f16 blocks + pad + tables
    "padded position 2^31 with BOTH f32 copies": (1 << 29) * (32 + 24),                  # 28 GiB
    "padded position 2^32 in the compact f32 copy": (1 << 30) * 24,                      # 24 GiB + pad + tables
}


# The search workspace: the smallest batch at k = 1024 for which a region of search_ws starts past byte 2^32, on the scaled-down
# build of p-f32-both (a 3 MB index: the workspace is what is large here), queries of one planted term each.
WS_K = 1024
WS_CASE = "p-f32-both"


def ws_plan(nq):
    c = next(x for x in CASES if x.name == WS_CASE)
    return parity.plan(c.n_tiles, c.unit_tiles, nq, WS_K, 0)


def ws_first_start_past(nq):
    """the first region of the workspace of an nq-query batch that starts past byte 2^32, or None"""
    w = parity.search_ws(ws_plan(nq), nq, WS_K)
    past = [name for name in ("cand_doc", "cand_score", "cand_count", "ovf", "done", "work") if w[name] > 1 << 32]
    return past[0] if past else None


def ws_nq():
    """With k = 1024 a query has at most 2 x 2 candidate lists of 1024 entries (4096 merge candidates): the lists take
    lists x 8192 bytes and the regions behind them start past 2^32 from about 131 000 queries on if the queries are split in
    two -- the plan says whether they are (a batch of a multiple of 3072 queries is not split).  Scanned upwards from a batch
    whose whole workspace ends below 2^32."""
    nq = (1 << 32) // (4 * (WS_K * 8 + 16))
    assert parity.plan_workspace_bytes(ws_plan(nq), nq, WS_K) < 1 << 32
    while ws_first_start_past(nq) is None:
        nq += 1
    return nq


WS_NQ2 = (1 << 32) // (4 * WS_K * 4) + 1  # 262 145: the first batch whose cand_score region STARTS past byte 2^32 (cand_doc lies across 2^31)


def ws_device_bytes(nq=WS_NQ2):
    return parity.plan_workspace_bytes(ws_plan(nq), nq, WS_K) + 4 * GUARD_WORDS + nq * (2 * WS_K + 1) * 4 + (64 << 20)


def arena_bytes():
    return r256(max(build(c).device_bytes() for c in CASES)) + (1 << 20)
