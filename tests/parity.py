"""Parity helpers shared by the CPU and GPU test suites.

Tie contract (oracle/bm25_oracle.c): the reference leaves the order of exactly equal
fp32 scores to NumPy's introselect/quicksort.  A result list therefore matches when
  * the score sequence is bit-identical,
  * inside every maximal run of equal scores the doc ids match as SETS, and
  * for the last run, if the list is full (count == k) the tie group may straddle rank k: then every
    doc we return in that run must be a doc whose true score equals the run's score (checked against
    the full score vector when one is supplied).
"""
import numpy as np


def runs(scores):
    out, s = [], 0
    for i in range(1, len(scores) + 1):
        if i == len(scores) or scores[i] != scores[s]:
            out.append((s, i))
            s = i
    return out


def assert_ranked_equal(got_docs, got_scores, exp_docs, exp_scores, k=None, full_scores=None, label=""):
    got_docs = np.asarray(got_docs)
    exp_docs = np.asarray(exp_docs)
    gs = np.asarray(got_scores, dtype=np.float32)
    es = np.asarray(exp_scores, dtype=np.float32)
    assert len(gs) == len(es), f"{label}: count {len(gs)} != {len(es)}"
    assert np.array_equal(gs.view(np.uint32), es.view(np.uint32)), f"{label}: scores differ\n{gs}\n{es}"
    assert np.all(gs[:-1] >= gs[1:]), f"{label}: not descending"
    rr = runs(es)
    for n, (a, b) in enumerate(rr):
        last_full = (n == len(rr) - 1) and (k is not None) and (len(es) == k)
        if not last_full:
            assert set(got_docs[a:b].tolist()) == set(exp_docs[a:b].tolist()), f"{label}: docs differ in run {a}:{b}"
        else:
            assert len(set(got_docs[a:b].tolist())) == b - a, f"{label}: duplicate docs in boundary run"
            if full_scores is not None:
                fs = np.asarray(full_scores, dtype=np.float32)
                for d in got_docs[a:b]:
                    assert fs[int(d)] == es[a], f"{label}: doc {d} in boundary tie run has score {fs[int(d)]} != {es[a]}"
    assert len(set(got_docs.tolist())) == len(got_docs), f"{label}: duplicate docs"


def assert_canonical_order(docs, scores, label=""):
    """Our own contract: (score desc, doc asc)."""
    d = np.asarray(docs, dtype=np.int64)
    s = np.asarray(scores, dtype=np.float32)
    for i in range(1, len(s)):
        assert s[i - 1] > s[i] or (s[i - 1] == s[i] and d[i - 1] < d[i]), f"{label}: order violated at {i}"


def np_build_blocks(indptr, indices, data, n_docs, vocab, tile_log2, unit_tiles, val_dtype=np.float32, block_pad=256):
    """NumPy restatement of the blocked posting layout (include/sparse_rx.h, srx_index_desc) from a doc-major CSR whose
    `data` are already the values to store.  Returns (term_ptr i64[V+1], post i32[(n_blocks+pad)*words],
    tile_skip i32[V*(n_tiles+1)], n_blocks).  Slow, small cases only: the checker of srx_build_blocks."""
    from scipy.sparse import csr_matrix
    m = csr_matrix((np.asarray(data, np.float32), np.asarray(indices), np.asarray(indptr)), shape=(n_docs, vocab)).tocsc()
    m.sort_indices()
    G = 1 << tile_log2
    n_tiles = (n_docs + G - 1) >> tile_log2
    U = unit_tiles * G
    n_units = (n_tiles + unit_tiles - 1) // unit_tiles
    words = 8 if val_dtype == np.float32 else 6
    term_ptr = np.zeros(vocab + 1, np.int64)
    skip = np.zeros((vocab, n_tiles + 1), np.int32)
    docs_out, vals_out = [], []
    pos = 0
    for t in range(vocab):
        term_ptr[t] = pos
        docs = m.indices[m.indptr[t]:m.indptr[t + 1]].astype(np.int64)
        vals = m.data[m.indptr[t]:m.indptr[t + 1]]
        start = pos
        unit_start = {}
        for u in range(n_units):
            sel = (docs >= u * U) & (docs < (u + 1) * U)
            unit_start[u] = pos - start
            d, v = docs[sel], vals[sel]
            padn = (-len(d)) % 4
            docs_out.append(np.concatenate([d, np.full(padn, -1 - 32 * (t % 64), np.int64)]))
            vals_out.append(np.concatenate([v, np.zeros(padn, np.float32)]))
            pos += len(d) + padn
        unit_start[n_units] = pos - start
        for j in range(n_tiles + 1):
            if j == n_tiles:
                skip[t, j] = pos - start
            else:
                u = j // unit_tiles
                skip[t, j] = unit_start[u] + int(((docs >= u * U) & (docs < j * G)).sum())
    term_ptr[vocab] = pos
    n_blocks = pos // 4
    dd = np.concatenate(docs_out + [np.repeat(-1 - 32 * (np.arange(block_pad, dtype=np.int64) % 64), 4)]).astype(np.int32).reshape(-1, 4)
    vv = np.concatenate(vals_out + [np.zeros(4 * block_pad, np.float32)]).astype(val_dtype).reshape(-1, 4)
    post = np.zeros((n_blocks + block_pad, words), np.int32)
    post[:, :4] = dd
    post[:, 4:] = vv.view(np.int32).reshape(n_blocks + block_pad, -1)
    return term_ptr, post.reshape(-1), skip.reshape(-1), n_blocks


def np_compact_blocks(post, unit_docs, val_dtype=np.float32):
    """NumPy restatement of the compact copy the tier-1 kernel streams (include/sparse_rx.h, srx_build_compact): per block
    four 16-bit unit-local doc ids (doc mod unit_docs; a sentinel -1 - 32 x becomes 49152 + 32 (x mod 64)) packed in two
    words, then the value words unchanged."""
    words = 8 if val_dtype == np.float32 else 6
    b = np.asarray(post, np.int32).reshape(-1, words)
    d = b[:, :4].astype(np.int64)
    loc = np.where(d >= 0, d % unit_docs, 49152 + 32 * (((-1 - d) >> 5) & 63)).astype(np.uint32)
    out = np.zeros((b.shape[0], words - 2), np.int32)
    out[:, 0] = (loc[:, 0] | (loc[:, 1] << 16)).astype(np.uint32).view(np.int32)
    out[:, 1] = (loc[:, 2] | (loc[:, 3] << 16)).astype(np.uint32).view(np.int32)
    out[:, 2:] = b[:, 4:]
    return out.reshape(-1)


# ---- the search planner, restated (csrc/sparse_rx.hip: make_plan, srx_search_workspace_bytes, search_impl) -----------------
# Constants of csrc/srx_common.h / sparse_rx.hip / merge.hip (srx_launch_final_merge).  The GPU tests pin this restatement to the library through
# DeviceIndex.workspace_bytes, which is a function of the plan: a planner change that moves a case to another bucket fails
# the case instead of letting it test something else silently.
PLAN_DEFAULT_TARGET = 3072  # make_plan: wave-sized work items per batch when target_blocks is 0
PLAN_MERGE_CANDIDATES = 4096  # MERGE_NPT * THREADS: the merge takes <= 4096 candidates (2 tiers x splits x k)
PLAN_MAX_TPS = 64  # MAX_TPS
W1_KMAX = 112  # largest k tier 1 ranks (larger k: every work item goes to tier 2)
W_KMAX = 128  # largest k the merge wave kernel ranks
MW_CAP = 1024  # merge wave kernel: lists_per_q * k candidates at most
W1_LCAP = 256  # tier 1's list capacity: the in-kernel merge selects down to k when count + c2 would exceed it
T2_GRID_MAX = 1024  # tier 2's persistent grid: min(items, 1024) workgroups ...
T2_GRID_SMALL = 128  # ... or 128 when the previous search of the index left the worklist empty


def plan(n_tiles, unit_tiles, nq, k, target_blocks=0):
    """make_plan for an index searched with the unit it was built for.  Returns a dict with n_super, n_splits, n_whole,
    lists_per_q, items (tier-1 work items = the grid of the wave kernel), ovf_words, merge_kernel ("wave" |
    "block" | None when no query is split), in_kernel_merge (the last split to arrive merges the query inside tier 1,
    unless a split handed work to tier 2), t2_everything (tier 1 ranks nothing: every item goes to tier 2) and t2_full
    (tier 2's full grid)."""
    tpu = min(max(int(unit_tiles), 1), PLAN_MAX_TPS)
    n_super = (int(n_tiles) + tpu - 1) // tpu
    target = target_blocks if target_blocks > 0 else PLAN_DEFAULT_TARGET
    ns = target // (nq if nq > 0 else 1)
    n_whole = 0
    if nq > target:
        n_whole = nq // target * target
        tail = nq - n_whole
        ns = target // tail if tail > 0 else 1
        ns = max(min(ns, 4), 2)
        if tail == 0:
            ns = 1
    ns = max(ns, 1)
    ns = min(ns, n_super)
    ns = min(ns, PLAN_MERGE_CANDIDATES // (2 * (k if k > 0 else 1)))
    ns = max(ns, 1)
    if ns == 1:
        n_whole = 0
    lists_per_q = 2 * ns
    merge = None
    if nq - n_whole > 0:
        merge = "wave" if (k <= W_KMAX and lists_per_q * k <= MW_CAP and lists_per_q <= 256) else "block"
    items = n_whole + (nq - n_whole) * ns
    return {"n_super": n_super, "n_splits": ns, "n_whole": n_whole, "tail": nq - n_whole if ns > 1 else 0,
            "lists_per_q": lists_per_q, "items": items, "ovf_words": (n_super + 31) // 32, "merge_kernel": merge,
            "in_kernel_merge": ns > 1 and k <= W1_KMAX, "t2_everything": k > W1_KMAX, "t2_full": min(items, T2_GRID_MAX)}


def plan_workspace_bytes(p, nq, k):
    """srx_search_workspace_bytes of a plan: candidate lists, counts, overflow bitmaps, arrival counters, worklist."""
    lists = nq * p["lists_per_q"]
    items = p["items"]
    return lists * k * 8 + lists * 4 + items * p["ovf_words"] * 4 + 4 * (1 + (nq - p["n_whole"])) + 4 * items + 256


def t2_grid(p, hint):
    """The tier-2 grid search_impl launches for plan `p` when the index's hint word (the worklist length of a recent
    search) reads `hint`."""
    return T2_GRID_SMALL if (hint == 0 and not p["t2_everything"] and p["t2_full"] > T2_GRID_SMALL) else p["t2_full"]


def plan_label(p, k):
    """A case's name in the bucket terms of the planner."""
    if p["n_splits"] == 1:
        shape = "whole"
    elif p["n_whole"] > 0:
        shape = f"mixed{p['n_whole']}+{p['tail']}x{p['n_splits']}"
    else:
        shape = f"split{p['n_splits']}"
    parts = [shape, f"k{k}"]
    if p["merge_kernel"]:
        parts.append(f"merge-{p['merge_kernel']}")
    if p["in_kernel_merge"]:
        parts.append("inkernel")
    if p["t2_everything"]:
        parts.append("t2all")
    return "-".join(parts)


# ---- the dense side, restated (csrc/dense.hip) --------------------------------------------------------------------------
# Dispatch: dense_qb, dense_splits, dense_sample, the first filter round's S1 and dense_ws (the workspace layout), with the
# constants of csrc/srx_common.h / dense.hip.  The GPU suite (test_dense_kernels.py) pins this to the library through
# srx_dense_workspace_bytes (QB through the score region, filtered-vs-matrix through the candidate buffers) and reads the
# overflow flags and survivor counts out of the workspace at the offsets restated here.
DENSE_DIMS = (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024)  # the INT8 kernels' instantiations: KS = dim / 32
DENSE_CAP = 65536  # candidate buffer entries per query of the filtered path
DENSE_CNT_STRIDE = 32  # ints between two queries' candidate counters
DENSE_SPLIT_DOCS = 256 * 16 * 4  # THREADS * DENSE_NPT * 4: docs per split of a score row at least
DENSE_MERGE_CANDIDATES = 4096  # MERGE_NPT * THREADS
F32_QP = 4  # queries per pass of the f32 / u8 matvec


def dense_qb(n_docs):
    """Queries per pass: the score matrix (queries x n_docs x 4 B) within 4 GiB, 32 .. 1024, a multiple of 32."""
    q = (4 << 30) // (((n_docs + 63) // 64 * 64) * 4)
    return int(min(max(q // 32 * 32, 32), 1024))


def dense_splits(n_docs, nq, k):
    """Doc-range splits of a score row: 2048 // nq, at most n_docs // 16384, at most one merge level (4096 // k)."""
    s = 2048 // (nq if nq > 0 else 1)
    s = min(s, n_docs // DENSE_SPLIT_DOCS, DENSE_MERGE_CANDIDATES // (k if k > 0 else 1))
    return max(s, 1)


def dense_sample(n_docs, k):
    """Sample size S of the threshold pass of the filtered path; 0 = the matrix path (n_docs < 65 536 or 4 S > n_docs)."""
    if n_docs < 65536:
        return 0
    S = (3 * k * n_docs + DENSE_CAP - 1) // DENSE_CAP
    S = max(S, min(max(164 * k, 4096), 16384))
    S = (S + 127) // 128 * 128
    return S if S * 4 <= n_docs else 0


def dense_ks_params(dim):
    """Per-instantiation constants of srx_dense_i8_filter_kernel<KS>: doc tiles per wave (DT), survivor list entries per
    wave (DENSE_CB), query tiles in LDS (NBUF), waves per workgroup (NW) and docs per workgroup."""
    ks = dim // 32
    nw = 4  # dense_filter_geom: four waves at every KS
    dt = 2 if ks <= 12 else 1
    cb = 512 if ks <= 12 else (256 if ks <= 24 else 128)
    nbuf = 3 if ks <= 16 else 2
    return {"KS": ks, "DT": dt, "DENSE_CB": cb, "NBUF": nbuf, "NW": nw, "docs_per_block": 32 * dt * nw}


def dense_s1(n_docs, S, dim):
    """Docs of the first filter round: sqrt(S n), rounded up to whole rounds of the chip (512 workgroups) once it reaches
    one, else to whole workgroups; n_docs (one round) when twice that exceeds the corpus.  Returns (S1, chip_rounded)."""
    import math
    dpb = dense_ks_params(dim)["docs_per_block"]
    s1 = int(math.sqrt(float(S) * float(n_docs)))
    chip = dpb * (2048 // 4)
    chip_rounded = s1 >= chip
    s1 = (s1 + chip - 1) // chip * chip if chip_rounded else (s1 + dpb - 1) // dpb * dpb
    if s1 * 2 > n_docs:
        return n_docs, False
    return s1, chip_rounded


def dense_ws(nq, n_docs, k):
    """dense_ws: byte offsets of the workspace regions (each rounded up to 256 B) and the total srx_dense_workspace_bytes."""
    QB = dense_qb(n_docs)
    qb = min(nq, QB)
    ld = (n_docs + 63) // 64 * 64
    ns = dense_splits(n_docs, qb, k)
    filt = dense_sample(n_docs, k) > 0
    off, w = 0, {}
    for name, nbytes in (("scores", qb * ld * 4), ("cand_doc", qb * ns * k * 4), ("cand_score", qb * ns * k * 4),
                         ("cand_count", qb * ns * 4), ("tau", qb * 4), ("buf_cnt", (qb * DENSE_CNT_STRIDE + qb + 1) * 4),
                         ("buf_doc", qb * DENSE_CAP * 4 if filt else 0), ("buf_score", qb * DENSE_CAP * 4 if filt else 0),
                         ("apack", (qb + 31) // 32 * 32 * 1024)):
        w[name] = off
        off += (nbytes + 255) // 256 * 256
    w["ovf"] = w["buf_cnt"] + qb * DENSE_CNT_STRIDE * 4
    w["any_ovf"] = w["ovf"] + qb * 4
    w["bytes"] = off + 256
    w["qb"] = qb
    return w


def dense_f32_ws_bytes(nq, n_docs, k):
    """srx_dense_f32_workspace_bytes: the score rows of one pass of F32_QP queries, their candidate lists and counts."""
    ld = (n_docs + 63) // 64 * 64
    ns = dense_splits(n_docs, F32_QP, k)
    return F32_QP * ld * 4 + F32_QP * ns * k * 8 + F32_QP * ns * 4 + 1024


def dense_plan(nq, n_docs, k, dim):
    """The dispatch of one srx_dense_search_i8 call: passes, path, rounds, S, S1 and the splits of the score-row ranking
    (the matrix path and the overflow fallback)."""
    QB = dense_qb(n_docs)
    S = dense_sample(n_docs, k)
    p = {"KS": dim // 32, "QB": QB, "passes": (nq + QB - 1) // QB, "S": S, "ns": dense_splits(n_docs, min(nq, QB), k),
         "path": "filtered" if S else "matrix", "rounds": 0, "S1": 0, "chip": False}
    if S:
        p["S1"], p["chip"] = dense_s1(n_docs, S, dim)
        p["rounds"] = 1 if p["S1"] >= n_docs else 2
    return p


def dense_plan_label(p, k):
    parts = [f"ks{p['KS']}", p["path"]]
    if p["path"] == "filtered":
        parts.append(f"r{p['rounds']}" + ("chip" if p["chip"] else ""))
    parts += [f"p{p['passes']}", f"ns{p['ns']}", f"k{k}"]
    return "-".join(parts)


def dense_rows_scores(rows, queries, scale_min=None, score_offset=0.0):
    """srx_dense_f32_scores_kernel / srx_dense_u8_scores_kernel restated bit for bit (fp32, no contraction): lane l of the
    doc's wave sums r[l + 64 i] * q[l + 64 i] over the 16 slices i in order (slices past dim / 64 add 0 * 0), the xor
    butterfly 32, 16, 8, 4, 2, 1 adds the lanes, lane 0's value + score_offset is the score.  u8 rows (scale_min given) are
    de-quantized first with one fp32 multiply and one add: u8 * scale_min[2 d] + scale_min[2 d + 1].
    rows f32 / u8 [n, dim], queries f32 [nq, dim], dim a multiple of 64 <= 1024.  Returns f32 [nq, n]."""
    f = np.float32
    q = np.asarray(queries, dtype=f)
    R = np.asarray(rows)
    n, dim = R.shape
    assert q.shape[1] == dim and dim % 64 == 0 and 0 < dim <= 1024
    nsl = dim // 64
    sm = None if scale_min is None else np.asarray(scale_min, dtype=f).reshape(-1)
    qv = q.reshape(len(q), nsl, 64)[:, None]  # [nq, 1, slice, lane]
    out = np.empty((len(q), n), f)
    chunk = max(1, (1 << 22) // (dim * max(1, len(q))))
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        r = R[lo:hi]
        if sm is None:
            r = r.astype(f, copy=False)
        else:
            r = r.astype(f) * sm[2 * lo:2 * hi:2, None] + sm[2 * lo + 1:2 * hi:2, None]
        r = r.reshape(hi - lo, nsl, 64)[None]  # [1, docs, slice, lane]
        a = np.zeros((len(q), hi - lo, 64), f)
        for i in range(nsl):
            a = a + r[:, :, i, :] * qv[:, :, i, :]
        if nsl < 16:
            a = a + f(0.0)  # the zero slices: -0 becomes +0, nothing else changes
        for o in (32, 16, 8, 4, 2, 1):  # lanes l and l ^ o hold the same sum after a step: lane 0's chain is this
            a = a[:, :, :o] + a[:, :, o:2 * o]
        out[:, lo:hi] = a[:, :, 0] + f(score_offset) if sm is None else a[:, :, 0]
    return out


def dense_topk_rows(similarities, k):
    """np_oracle.dense_topk (score > 0 only, (score desc, doc asc), padded with -1 / 0) through a partition: only the
    candidates at or above each row's k-th largest value are sorted.  Same rows; fast on wide corpora."""
    s = np.asarray(similarities, dtype=np.float32)
    nq, n = s.shape
    out_d = np.full((nq, k), -1, np.int32)
    out_s = np.zeros((nq, k), np.float32)
    out_n = np.zeros(nq, np.int32)
    kk = min(k, n)
    thr = -np.partition(-s, kk - 1, axis=1)[:, kk - 1]
    for i in range(nq):
        c = np.flatnonzero((s[i] >= thr[i]) & (s[i] > 0))
        c = c[np.lexsort((c, -s[i, c].astype(np.float64)))][:k]
        out_d[i, : len(c)] = c
        out_s[i, : len(c)] = s[i, c]
        out_n[i] = len(c)
    return out_d, out_s, out_n


# ---- tier 1's hand-over rules, restated (csrc/wave_kernel.hip, csrc/sparse_rx.hip: search_ws) -----------------------------
# After a search the caller's workspace still holds what tier 1 decided: ovf[items][ovf_words], one bit per (work item,
# global unit index) that tier 1 left to tier 2, and the worklist work[0] (its length), work[1 ..] (the items on it).  The
# route tests (test_tier1_routes_gpu.py) read both and compare them with tier1_routes below.
W_MAXT = 64  # query terms tier 1 serves
W_R = 12  # postings per lane per unit: a term's run of more than 3 LPT blocks does not fit the registers
W_DUPCAP = 48  # multi-term resolution visits per unit (the 49th rolls the unit back)
W_UNIT_MAX_DOCS = 49152
BOUND_KS = (1, 10, 100, 1000)  # the ranks of the term_bound columns


def search_ws(p, nq, k):
    """search_ws of sparse_rx.hip: byte offsets of the regions of a search's workspace for plan `p`, and `end` (the first
    byte behind the worklist; end + 256 = srx_search_workspace_bytes)."""
    lists = nq * p["lists_per_q"]
    items = p["items"]
    w, off = {}, 0
    for name, nbytes in (("cand_doc", lists * k * 4), ("cand_score", lists * k * 4), ("cand_count", lists * 4),
                         ("ovf", items * p["ovf_words"] * 4), ("done", (nq - p["n_whole"]) * 4), ("work", (1 + items) * 4)):
        w[name] = off
        off += nbytes
    w["end"] = off
    return w


def item_of(p, q, split):
    """decode_item inverted: the work item of (query, split).  The first n_whole queries are one item each."""
    if q < p["n_whole"]:
        assert split == 0
        return q
    return p["n_whole"] + (q - p["n_whole"]) * p["n_splits"] + split


def item_queries(p, nq):
    """decode_item for every work item: (q i64[items], split i64[items], nsq i64[items])."""
    it = np.arange(p["items"], dtype=np.int64)
    j = np.maximum(it - p["n_whole"], 0)
    whole = it < p["n_whole"]
    q = np.where(whole, it, p["n_whole"] + j // p["n_splits"])
    split = np.where(whole, 0, j % p["n_splits"])
    nsq = np.where(whole, 1, p["n_splits"])
    assert np.all(q < nq)
    return q, split, nsq


def bound_column_of(k):
    """bound_column of srx_common.h: the column of term_bound valid for top-k k (-1: none)."""
    return 0 if k <= 1 else 1 if k <= 10 else 2 if k <= 100 else 3 if k <= 1000 else -1


def stored_values(indptr, data, doc_lengths, mode="bm25", val_dtype="f32", k1=1.2, b=0.75, avgdl=1.0):
    """The value the index stores for every CSR entry: the oracle's fp32 impact (bm25) or the entry itself, through fp16
    when the index keeps fp16 values (dot mode only)."""
    data = np.asarray(data, np.float32)
    if mode == "bm25":
        from oracle import np_oracle
        rows = np.repeat(np.arange(len(indptr) - 1), np.diff(np.asarray(indptr)))
        return np_oracle.impacts_f32(data, rows, doc_lengths, k1, b, avgdl).astype(np.float32)
    return data.astype(np.float16).astype(np.float32) if val_dtype == "f16" else data


def tier1_routes(indptr, indices, data, doc_lengths, idf, q, tile_log2, unit_tiles, k, p, term_bound=True, mode="bm25",
                 val_dtype="f32", k1=1.2, b=0.75, avgdl=1.0):
    """Tier 1's hand-over rules for every (work item, unit) of one search: which units it MUST flag for tier 2, which it
    MUST serve itself, and which MAY go either way.  q = (q_ptr, q_term, q_weight) with the terms in the order the kernel
    accumulates them; p = plan().  Returns a dict of
      nt[items], all_t2[items]  -- nt > 64 or k > 112 (or a unit too large for 16-bit local ids): the item is on the
                                   worklist when nt > 0 and its flag words stay 0;
      in_range[items, n_super]  -- the unit belongs to the item's [su_lo, su_hi);
      must_flag, must_serve, may [items, n_super] -- a partition of in_range for the items tier 1 serves (nt > 0):
        must_flag : some term has ceil(cnt / 4) > 3 LPT blocks in the unit (LPT = 64 >> ceil(log2 nt)), or the unit needs
                    sum over docs of (m_d - 1) >= 49 resolution visits (m_d = query terms with a non-zero stored value);
        must_serve: not must_flag and k + E <= 256, E = docs of the unit with exact fp32 score > 0 and >= tau0 (the list
                    takes at most one entry per such doc and tau never falls below tau0, the kernel's initial threshold);
        may       : the rest -- whether the list has room depends on its state.
      tau0[nq] (fp32)."""
    from scipy.sparse import csr_matrix
    import oracle
    f = np.float32
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int32)
    data = np.asarray(data, np.float32)
    idf = np.asarray(idf, np.float32)
    q_ptr, q_term, q_w = (np.asarray(x) for x in q)
    q_w = q_w.astype(np.float32)
    nq = len(q_ptr) - 1
    n_docs, V = len(indptr) - 1, len(idf)
    unit_docs = unit_tiles << tile_log2
    n_super = p["n_super"]
    n_tiles = (n_docs + (1 << tile_log2) - 1) >> tile_log2
    assert n_super == (n_tiles + unit_tiles - 1) // unit_tiles, "the plan is of another index"
    sv = stored_values(indptr, data, doc_lengths, mode, val_dtype, k1, b, avgdl)
    csc = csr_matrix((sv, indices, indptr), shape=(n_docs, V)).tocsc()  # explicit zeros stay: they are postings
    csc.sort_indices()
    bounds_on = bool(term_bound) and bound_column_of(k) >= 0 and not np.any(sv < 0)
    K = BOUND_KS[bound_column_of(k)] if bounds_on else 0
    sdata = sv if mode == "dot" else data  # the oracle computes the impact itself; in dot mode it gets the stored (fp16-exact) values

    q_of, split_of, nsq_of = item_queries(p, nq)
    items = p["items"]
    nt_q = np.diff(q_ptr).astype(np.int64)
    out = {"nt": nt_q[q_of], "in_range": np.zeros((items, n_super), bool), "tau0": np.zeros(nq, f)}
    out["all_t2"] = (out["nt"] > W_MAXT) | (k > W1_KMAX) | (unit_docs > W_UNIT_MAX_DOCS)
    per_q = {}
    for qi in range(nq):
        nt = int(nt_q[qi])
        if nt == 0 or nt > W_MAXT or k > W1_KMAX or unit_docs > W_UNIT_MAX_DOCS:
            continue
        terms = q_term[q_ptr[qi]:q_ptr[qi + 1]]
        w = q_w[q_ptr[qi]:q_ptr[qi + 1]]
        lg = 0
        while (1 << lg) < nt:
            lg += 1
        lpt = 64 >> lg
        long_run = np.zeros(n_super, bool)
        m = np.zeros(n_docs, np.int64)
        tau0, neg = f(0.0), False
        for t, wt in zip(terms, w):
            docs = csc.indices[csc.indptr[t]:csc.indptr[t + 1]]
            vals = csc.data[csc.indptr[t]:csc.indptr[t + 1]]
            cnt = np.bincount(docs // unit_docs, minlength=n_super)
            long_run |= (cnt + 3) // 4 > (W_R // 4) * lpt
            np.add.at(m, docs[vals != 0], 1)
            neg = neg or idf[t] < 0 or wt < 0
            if bounds_on and idf[t] > 0 and wt > 0:
                pos = np.sort(vals[vals > 0])[::-1]
                bnd = pos[K - 1] if len(pos) >= K else f(0.0)
                tau0 = max(tau0, f(0.0) + (f(bnd) * idf[t]) * f(wt))
        tau0 = f(0.0) if neg else f(tau0)
        out["tau0"][qi] = tau0
        unit_of = np.arange(n_docs) // unit_docs
        visits = np.bincount(unit_of, weights=np.maximum(m - 1, 0), minlength=n_super).astype(np.int64)
        matched = np.bincount(unit_of, weights=(m > 0), minlength=n_super).astype(np.int64)
        flag = long_run | (visits > W_DUPCAP)
        E = matched.copy()
        if np.any(~flag & (k + matched > W1_LCAP)):  # only then does the exact count matter: E <= matched
            s = oracle.scores_given_order(indptr, indices, sdata, doc_lengths, idf, terms.astype(np.int32), w, k1, b, avgdl, tfidf=(mode == "dot"))
            E = np.bincount(unit_of, weights=((s > 0) & (s >= tau0)), minlength=n_super).astype(np.int64)
        per_q[qi] = (flag, ~flag & (k + E <= W1_LCAP))
    must_flag = np.zeros((items, n_super), bool)
    must_serve = np.zeros((items, n_super), bool)
    for it in range(items):
        lo = n_super * int(split_of[it]) // int(nsq_of[it])
        hi = n_super * (int(split_of[it]) + 1) // int(nsq_of[it])
        out["in_range"][it, lo:hi] = True
        if int(q_of[it]) in per_q:
            fl, srv = per_q[int(q_of[it])]
            must_flag[it, lo:hi] = fl[lo:hi]
            must_serve[it, lo:hi] = srv[lo:hi]
    served_item = (~out["all_t2"] & (out["nt"] > 0))[:, None]
    out["must_flag"], out["must_serve"] = must_flag, must_serve
    out["may"] = out["in_range"] & served_item & ~must_flag & ~must_serve
    return out


def decode_routes(ws_bytes, p, nq, k):
    """The flags and the worklist out of a workspace (a uint8 array) after a search: (ovf bool[items, 32 ovf_words] -- bit su
    of item i --, the items on tier 2's worklist in list order, the list's length work[0])."""
    w = search_ws(p, nq, k)
    words = np.frombuffer(ws_bytes.tobytes(), dtype=np.uint32)
    ovf = words[w["ovf"] // 4: w["ovf"] // 4 + p["items"] * p["ovf_words"]].reshape(p["items"], p["ovf_words"])
    bits = ((ovf[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).astype(bool).reshape(p["items"], -1)
    work = words[w["work"] // 4: w["work"] // 4 + 1 + p["items"]].view(np.int32)
    n = int(work[0])
    assert 0 <= n <= p["items"], f"work[0] = {n} with {p['items']} items"
    return bits, work[1:1 + n].tolist(), n


# ---- tier 2's dispatch, restated (csrc/tier2_kernel.hip: score_block and what it calls; csrc/srx_common.h) ---------------
# Which of its paths the tier-2 kernel takes for every unit of every work item, and what its selection sites then do.  The
# path cannot be observed from outside the kernel: tests/test_tier2_routes_cpu.py builds corpora that sit on each comparison
# below and asserts through tier2_routes that they do; tests/test_tier2_routes_gpu.py runs them bit for bit against the oracle.
# Every constant is named as in C++ and pinned to the sources by test_tier2_constants_match_the_sources.
THREADS = 256
TBL_WORDS = 16384
SLOTS = 8192  # TBL_WORDS / 2
HASH_CAP = 4096
DENSE_MIN = 4096  # = HASH_CAP
KMAX = 1024  # = SRX_MAX_K
MAXT = 256
MAX_TPS = 64
OVF_CAP = 384
FLAT_CAP = 8192
FLAT_MCAP = 2048
FLAT_MIN_TERMS = 12
WAVES = 4  # THREADS / 64
SRX_DBG_TIER2_ONLY, SRX_DBG_NO_TERM_BOUND, SRX_DBG_NO_FLAT_TILES = 8, 16, 128
SRX_DBG_NO_WAVE_DENSE, SRX_DBG_WAVE_DENSE_MASKED, SRX_DBG_WAVE_DENSE_GENERAL = 2048, 4096, 8192


def hash_slot(doc):
    """hash_unit's home slot of a doc: (doc * 0x9E3779B1 mod 2^32) >> (32 - 13)."""
    return ((np.asarray(doc, np.int64) * 0x9E3779B1) & 0xFFFFFFFF) >> 19


def tier1_cannot_serve(nt, k, tps, tile_log2, vocab, n_tiles, dbg, post16=True):
    """srx_common.h: tier1_cannot_serve.  dbg is the launch's (search_impl adds SRX_DBG_TIER2_ONLY for a unit override, a
    search-after and a filtered search)."""
    return (nt > W_MAXT or k > W1_KMAX or (tps << tile_log2) > W_UNIT_MAX_DOCS or not post16 or (dbg & SRX_DBG_TIER2_ONLY) != 0
            or vocab * (n_tiles + 1) >= (1 << 30))


class _T2List:
    """The work item's running list, simulated exactly: the docs on it, tau, and the cut every selection site shares (the k
    best in (score desc, doc asc) order, tau = the k-th score)."""

    def __init__(self, s, tau0, k, bound, allowed=None):
        self.s, self.tau, self.k, self.bound, self.allowed = s, np.float32(tau0), k, bound, allowed
        self.docs = np.zeros(0, np.int64)
        self.log = []  # per fold / dense_group call: (outcome, the docs it counted: the list's, then the candidates)

    def cand(self, docs):
        """The docs of `docs` that can enter: score > 0, bits >= tau (float order for positive scores), after the bound, then
        the filter bit (tier2_filter.hip's predicate: the bound first, then the row)."""
        docs = np.asarray(docs, np.int64)
        sc = self.s[docs]
        ok = (sc > 0) & (sc >= self.tau)
        if self.bound is not None:
            ub, ud = self.bound
            ok &= (sc < ub) | ((sc == ub) & (docs > ud))
        if self.allowed is not None:
            ok &= self.allowed[docs]
        return docs[ok]

    def select(self, extra=()):
        d = np.concatenate([self.docs, np.asarray(extra, np.int64)])
        d = d[np.lexsort((d, -self.s[d].astype(np.float64)))][: self.k]
        self.docs, self.tau = d, self.s[d[-1]]

    def _logged(self, c, outcome):
        self.log.append((outcome, np.concatenate([self._before, c])))
        return outcome

    def fold(self, docs, cap=KMAX):
        """topk_fold<N, LAZY>: nothing / append while the list has room / the selection."""
        self._before = self.docs
        return self._logged(self.cand(docs), self._fold(docs, cap))

    def _fold(self, docs, cap):
        c = self.cand(docs)
        n_old, n_new = len(self.docs), len(c)
        if n_new == 0 and n_old <= self.k:
            return ("fold_none", n_old)
        if n_old + n_new <= cap:
            self.docs = np.concatenate([self.docs, c])
            return ("fold_append", n_old + n_new)
        self.select(c)
        return ("fold_select", n_old + n_new)

    def dense_group(self, lo, hi, n_docs, append_scan, ovf_cap):
        """One dense group [lo, hi) of docs: dense_tile_append, then dense_tile_general when it refuses."""
        self._before = self.docs
        return self._logged(self.cand(np.arange(lo, min(hi, n_docs))), self._dense_group(lo, hi, n_docs, append_scan, ovf_cap))

    def _dense_group(self, lo, hi, n_docs, append_scan, ovf_cap):
        rng = np.arange(lo, min(hi, n_docs))
        if append_scan:
            n_old = len(self.docs)
            for attempt in range(2):
                c = self.cand(rng)
                if n_old + len(c) <= KMAX + ovf_cap:
                    self.docs = np.concatenate([self.docs, c])
                    return ("append_served", n_old + len(c)) if attempt == 0 else ("append_retry_served", n_old + len(c))
                if n_old <= self.k:
                    break
                self.select()  # list_compact_select(k, n_old)
                n_old = self.k
        c = self.cand(rng)  # dense_tile_general
        n_old, n_new = len(self.docs), len(c)
        pre = "append_refused -> " if append_scan else ""
        if n_new == 0 and n_old <= self.k:
            return (pre + "early_return", n_old)
        if n_old + n_new <= KMAX:
            self.docs = np.concatenate([self.docs, c])
            return (pre + "general_append", n_old + n_new)
        self.select(c)
        return (pre + "general_cut", n_old + n_new)


def tier2_routes(indptr, indices, data, doc_lengths, idf, q, tile_log2, unit_tiles, k, p, debug, flags, tps=None, mode="bm25",
                 val_dtype="f32", k1=1.2, b=0.75, avgdl=1.0, post16=True, after=None, layout=None, allowed=None):
    """What score_block does for every work item of one search, as an ordered list of steps per item.
    unit_tiles = the unit the index was built (padded) for, tps = tiles per unit of the search (the plan's; default the same),
    p = plan(n_tiles, tps, ...), debug = the search's debug bits, flags = bool[items, >= n_super] tier 1's flag bits (from
    tier1_routes on the CPU, from decode_routes on the GPU), after = None or (score f32[nq], shard-local doc[nq]) of a search-
    after page, layout = (term_ptr, post, tile_skip, n_blocks) of np_build_blocks on the stored values (built here when None).
    Steps (tuples):
      ("skip",)                                              not opened: no flagged unit, or nt == 0
      ("many_term", ja, jb, n_pass, last_pass_terms, [sel])  nt > 256; one selection outcome per tile (ovf_cap = 0)
      ("quads_all", ja, jb, masked, [sel], compact)          tier1_cannot_serve and the wave-level dense path
      (su, "empty") | (su, "flat", P, M, [fold, fold]) | (su, "flat_refused", P, M) then what serves the unit |
      (su, "hash", P, n_steps, fold) | (su, "quads_unit", ja, jb, masked, [sel], compact) |
      (su, "packed", [(tiles, GP, "hash" | "dense" | "empty", outcome), ...])
      ("t1_fold", c1, passed, tau, fold)                     unsplit query whose other units tier 1 served: tier 1's c1 entries, how
                                                             many reach tier 2's tau, the fold's outcome (before "emit")
      ("emit", entries, shrunk)                              topk_shrink ran a selection or not
    A selection outcome is (name, n) with the names of _T2List; `compact` says whether list_compact_select ran at the end of
    dense_quads.  Also returned per item: tau0 and all_units.
    allowed = None, or one entry per query -- None (the query's filter row is -1) or bool[n_docs] over local docs -- of a
    FILTERED search: search_impl then sends everything to tier 2 and drops the term bounds for every query of the batch
    (tau0 = 0), and the mask joins the candidate predicate (_T2List.cand) and nothing else: P, M, n_steps, the packer's groups
    and `masked` are functions of the postings.  With `allowed` the result also carries "sel_docs": per item, for every
    selection outcome in step order, (outcome, the docs the decision counted: those on the list, then the candidates)."""
    from scipy.sparse import csr_matrix
    import oracle
    f = np.float32
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int32)
    data, idf = np.asarray(data, np.float32), np.asarray(idf, np.float32)
    q_ptr, q_term, q_w = (np.asarray(x) for x in q)
    q_w = q_w.astype(np.float32)
    nq, n_docs, V = len(q_ptr) - 1, len(indptr) - 1, len(idf)
    tps = unit_tiles if tps is None else tps
    G = 1 << tile_log2
    n_tiles = (n_docs + G - 1) >> tile_log2
    n_super = p["n_super"]
    assert n_super == (n_tiles + tps - 1) // tps, "the plan is of another search"
    sv = stored_values(indptr, data, doc_lengths, mode, val_dtype, k1, b, avgdl)
    if layout is None:
        layout = np_build_blocks(indptr, indices, sv, n_docs, V, tile_log2, unit_tiles)
    term_ptr, post, skip = layout[0], layout[1].reshape(-1, 8), layout[2].reshape(V, n_tiles + 1)
    post_doc = post[:, :4].reshape(-1)  # the doc of posting position g (negative: run padding)
    csc = csr_matrix((sv, indices, indptr), shape=(n_docs, V)).tocsc()
    sdata = sv if mode == "dot" else data
    filtered = allowed is not None
    assert not filtered or len(allowed) == nq, "one mask (or None) per query"
    dbg = debug | (SRX_DBG_TIER2_ONLY if (after is not None or filtered or tps != unit_tiles) else 0)  # search_impl: restricted
    col = bound_column_of(k)
    bounds_on = not (dbg & SRX_DBG_NO_TERM_BOUND) and after is None and not filtered and col >= 0 and not np.any(sv < 0)  # index_view
    q_of, split_of, nsq_of = item_queries(p, nq)
    flags = np.asarray(flags, bool)
    out = {"steps": [], "tau0": [], "all_units": []}
    if filtered:
        out["sel_docs"] = []
    per_q = {}
    for it in range(p["items"]):
        qi, split, nsq = int(q_of[it]), int(split_of[it]), int(nsq_of[it])
        terms = q_term[q_ptr[qi]:q_ptr[qi + 1]].astype(np.int64)
        w = q_w[q_ptr[qi]:q_ptr[qi + 1]]
        nt = len(terms)
        su_lo, su_hi = n_super * split // nsq, n_super * (split + 1) // nsq
        all_units = tier1_cannot_serve(nt, k, tps, tile_log2, V, n_tiles, dbg, post16)
        any_ = all_units and nt > 0
        if not all_units and nt > 0 and su_lo < su_hi:  # whole flag words, as the kernel reads them
            any_ = bool(flags[it, (su_lo >> 5) * 32: ((su_hi - 1) >> 5) * 32 + 32].any())
        out["all_units"].append(all_units)
        if not any_:
            out["steps"].append([("skip",)])
            out["tau0"].append(f(0))
            if filtered:
                out["sel_docs"].append([])
            continue
        if qi not in per_q:  # open_item's tau0, the exact scores in the kernel's order, postings per doc
            tau0, neg, nonfinite = f(0), False, False
            m = np.zeros(n_docs, np.int64)
            for t, wt in zip(terms, w):
                vals = csc.data[csc.indptr[t]:csc.indptr[t + 1]]
                np.add.at(m, csc.indices[csc.indptr[t]:csc.indptr[t + 1]], 1)
                nonfinite = nonfinite or not (abs(idf[t]) <= 3.0e38) or not (abs(wt) <= 3.0e38)
                if idf[t] < 0 or wt < 0:
                    neg = True
                elif bounds_on and idf[t] > 0 and wt > 0:
                    pos = np.sort(vals[vals > 0])[::-1]
                    K = BOUND_KS[col]
                    bnd = pos[K - 1] if len(pos) >= K else f(0)
                    bb = f(0) + (f(bnd) * idf[t]) * f(wt)
                    tau0 = max(tau0, bb if bb > 0 else f(0))
            tau0 = f(0) if (neg or nonfinite or after is not None) else f(tau0)
            with np.errstate(all="ignore"):
                s = oracle.scores_given_order(indptr, indices, sdata, doc_lengths, idf, terms.astype(np.int32), w, k1, b, avgdl, tfidf=(mode == "dot"))
            per_q[qi] = (tau0, nonfinite, s, m)
        tau0, nonfinite, s, m = per_q[qi]
        out["tau0"].append(tau0)
        L = _T2List(s, tau0, k, None if after is None else (f(max(after[0][qi], 0)), int(after[1][qi])),
                    None if not filtered or allowed[qi] is None else np.asarray(allowed[qi], bool))
        append_scan = not (dbg & SRX_DBG_WAVE_DENSE_GENERAL)
        steps = []

        def emit():
            n = len(L.docs)
            if n > k:
                L.select()
            if nsq == 1 and not all_units:
                # emit_item on an unsplit query: tier 1's list of the same query -- the k best of the docs of the units it
                # served (exact only where tier 1's threshold starts at 0: debug 16) -- is folded in: its first min(count, k)
                # entries, those with bits >= tau and != 0, through topk_fold<KPT, false> (capacity k)
                served = np.flatnonzero(~flags[it, :n_super])
                d1 = np.concatenate([np.arange(u * tps * G, min((u + 1) * tps * G, n_docs)) for u in served] + [np.zeros(0, np.int64)]).astype(np.int64)
                d1 = d1[s[d1] > 0]
                d1 = d1[np.lexsort((d1, -s[d1].astype(np.float64)))][:k]
                tau_emit = L.tau
                ok = d1[s[d1] >= tau_emit]
                steps.append(("t1_fold", len(d1), len(ok), float(tau_emit), L.fold(ok, cap=k)[0]))
            steps.append(("emit", n, n > k))
            out["steps"].append(steps)
            if filtered:
                out["sel_docs"].append(L.log)

        if nt > MAXT:
            ja, jb = su_lo * tps, min(su_hi * tps, n_tiles)
            sel = [L.dense_group(j * G, (j + 1) * G, n_docs, append_scan, 0) for j in range(ja, jb)]
            steps.append(("many_term", ja, jb, (nt + MAXT - 1) // MAXT, nt - (nt - 1) // MAXT * MAXT, sel))
            emit()
            continue
        wave_dense = (4 << tile_log2) <= TBL_WORDS and nt <= 64 and not (dbg & SRX_DBG_NO_WAVE_DENSE)
        masked = not (unit_tiles == 1 and not nonfinite and not (dbg & SRX_DBG_WAVE_DENSE_MASKED))

        def dense_quads(ja, jb):
            # a wave whose tile is at or beyond jb zeroes its accumulators and adds nothing: the scan sees the tiles below jb only
            sel = [L.dense_group(j0 * G, min(j0 + WAVES, jb) * G, n_docs, append_scan, OVF_CAP) for j0 in range(ja, jb, WAVES)]
            compact = len(L.docs) > KMAX
            if compact:
                L.select()
            return ja, jb, masked, sel, compact

        def hash_unit(ja, jb):  # the unit's candidates are the docs of its tiles: a doc without a posting scores 0
            return L.fold(np.arange(ja * G, min(jb * G, n_docs)))

        if all_units and wave_dense:
            steps.append(("quads_all",) + dense_quads(su_lo * tps, min(su_hi * tps, n_tiles)))
            emit()
            continue
        for su in range(su_lo, su_hi):
            if not all_units and not flags[it, su]:
                continue
            ja, jb = su * tps, min(su * tps + tps, n_tiles)
            lens = skip[terms, min(ja + tps, n_tiles)] - skip[terms, min(ja, n_tiles)]
            P = int(lens.sum())
            if P == 0:
                steps.append((su, "empty"))
                continue
            if tps == 1 and nt >= FLAT_MIN_TERMS and P <= FLAT_CAP and not (dbg & SRX_DBG_NO_FLAT_TILES):
                docs = np.concatenate([post_doc[term_ptr[t] + skip[t, ja]: term_ptr[t] + skip[t, ja] + n] for t, n in zip(terms, lens)])
                docs = docs[docs >= 0]
                M = int((m[docs] >= 2).sum())
                if M <= FLAT_MCAP:
                    u = np.unique(docs)
                    steps.append((su, "flat", P, M, [L.fold(u[m[u] == 1]), L.fold(u[m[u] >= 2])]))
                    continue
                steps.append((su, "flat_refused", P, M))
            if P <= DENSE_MIN:
                steps.append((su, "hash", P, int(((lens + THREADS - 1) // THREADS).sum()), hash_unit(ja, jb)))
            elif wave_dense:
                steps.append((su, "quads_unit") + dense_quads(ja, jb))
            else:  # packed_unit: greedy groups of whole tiles
                ptile = [int((skip[terms, ja + j + 1] - skip[terms, ja + j]).sum()) for j in range(jb - ja)]
                grp, acc_p = [0], 0
                for j, pj in enumerate(ptile):
                    if acc_p > 0 and acc_p + pj > DENSE_MIN:
                        grp.append(j)
                        acc_p = 0
                    acc_p += pj
                grp.append(jb - ja)
                groups = []
                for ga, gb in zip(grp[:-1], grp[1:]):
                    GP = int((skip[terms, ja + gb] - skip[terms, ja + ga]).sum())
                    if GP == 0:
                        groups.append(((ja + ga, ja + gb), 0, "empty", None))
                    elif GP <= DENSE_MIN:
                        groups.append(((ja + ga, ja + gb), GP, "hash", hash_unit(ja + ga, ja + gb)))
                    else:  # one tile above DENSE_MIN, the group's last: only empty tiles can come before it (acc_p == 0 never closes a group)
                        assert sum(ptile[ga:gb - 1]) == 0 and ptile[gb - 1] == GP
                        groups.append(((ja + ga, ja + gb), GP, "dense", L.dense_group((ja + gb - 1) * G, (ja + gb) * G, n_docs, append_scan, 0)))
                steps.append((su, "packed", groups))
        emit()
    return out
