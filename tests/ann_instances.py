"""The kernel instances and loop shapes of the three list / product-code units (dense_pq.hip, dense_ivf.hip, dense_ivfpq.hip) as a
table: per unit the dispatch and plan rules of the host side restated in Python (each with its source line quoted), the GPU cases
of tests/test_ann_instances_gpu.py as plain tuples, and the shapes the units' own test files already run.  A plain module, as the
``*_ref.py`` files are: it never imports the package.  tests/test_ann_instances_cpu.py parses the dispatch lines of the kernel
sources and asserts that these cases and the existing shapes together reach every instantiated kernel and every loop shape named
there; the GPU file parametrizes over these lists and over nothing else, so the two cannot drift apart.

A new instance on a dispatch line needs a case here before the CPU test passes again."""

BASE = 3_000_000                 # the doc_base of the cases that have one
CUS = 256                        # compute units of the MI355X
CU_SPREAD = (64, 80, 104, 120, 128, 192, 228, 256, 304, 320)  # other counts the persistent-grid cases must hold for
PASS = 1024                      # the cap of every pass plan: half_plan's QB, IVF_PASS, IVFPQ_PASS


def ceil_div(a, b):
    return -(-a // b)


def r256(x):
    return ceil_div(x, 256) * 256


def subspaces(dim, dsub):
    """`*M = (dim + dsub - 1) / dsub;`"""
    return ceil_div(dim, dsub)


def pieces(M):
    """`inline int pq_pieces(int M) { return (M + 15) / 16; }`, ivfpq_pieces alike"""
    return (M + 15) // 16


def merge_bytes(n_rows, n_lists, k):
    """srx_merge_workspace_bytes as ivf.py and ivfpq.py restate it: nothing for one merge level"""
    g = ceil_div(n_lists, 4096 // k)
    return 2 * (n_rows * g * k * 8 + n_rows * g * 4 + 256) if g > 1 else 0


def scorer_grid(m):
    """(gridDim.y, trips of thread 0 of chunk 0) of srx_pq_score_docs_kernel and srx_ivfpq_score_docs_kernel:
    `const int64_t chunks = ((int64_t)m + PQ_DOCS_CHUNK - 1) / PQ_DOCS_CHUNK;` (8 * 1024 candidates),
    `const dim3 grid((unsigned)nq, (unsigned)(chunks < 64 ? chunks : 64));`,
    `for (int64_t c = (int64_t)blockIdx.y * PQ_SCAN_THREADS + tid; c < a.m; c += (int64_t)gridDim.y * PQ_SCAN_THREADS)`"""
    gy = min(ceil_div(m, 8192), 64)
    return gy, ceil_div(m, gy * 1024)


# =================================================================================================== dense_pq.hip
PQ_SCAN_KIB = 144  # `constexpr int PQ_SCAN_FLOATS = 144 * 256;`: KiB of tables in LDS, one KiB per subspace and query


def pq_scan_threads(np_):
    """`constexpr int pq_scan_threads(int np) { return np < 8 ? PQ_SCAN_THREADS : PQ_SCAN_THREADS / 2; }`"""
    return 1024 if np_ < 8 else 512


def half_plan(nq, n_docs, k):
    """(QB, qb_max, ld, ns) of half_common.h's half_plan, the pass plan of srx_pq_search:
    `p.ld = (n_docs + 63) / 64 * 64;`  `const int64_t q = (4ll << 30) / (p.ld * 4) / 32 * 32;`
    `p.QB = (int)(q < 32 ? 32 : q > 1024 ? 1024 : q);`  `p.qb_max = nq < p.QB ? nq : p.QB;`
    `int64_t s = 2048 / (p.qb_max > 0 ? p.qb_max : 1);`
    `const int64_t by_docs = n_docs / (THREADS * HF_NPT * 4), cap = (MERGE_NPT * THREADS) / (k > 0 ? k : 1);` (16384 docs, 4096 / k)"""
    ld = ceil_div(n_docs, 64) * 64
    QB = min(max((4 << 30) // (ld * 4) // 32 * 32, 32), PASS)
    qb_max = min(nq, QB)
    ns = max(1, min(2048 // max(qb_max, 1), n_docs // 16384, 4096 // k))
    return QB, qb_max, ld, ns


def pq_workspace_bytes(nq, n_docs, M, k):
    """pq_ws: `w.lut = take(qb_max * M * 1024)`, `w.scores = take(qb_max * ld * 4)`, the lists of k, `+ 256`"""
    _, qb, ld, ns = half_plan(nq, n_docs, k)
    return r256(qb * M * 1024) + r256(qb * ld * 4) + 2 * r256(qb * ns * k * 4) + r256(qb * ns * 4) + 256


def pq_passes(nq, n_docs, k=10):
    """[queries of every pass]: `for (int q0 = 0; q0 < nq; q0 += p.QB)`"""
    QB = half_plan(nq, n_docs, k)[0]
    return [min(QB, nq - q0) for q0 in range(0, nq, QB)]


def pq_scan_plan(qb, n_docs, M, cus):
    """(qg, n_groups, blocks_per_group, stride in tiles, n_tiles) of one pass of qb queries:
    `const int qg_max = PQ_SCAN_FLOATS / (M * 256);`  `const int qg = qb < qg_max ? qb : qg_max, n_groups = (qb + qg - 1) / qg;`
    `int64_t bpg = (2 * (int64_t)(n_cus > 0 ? n_cus : 1) + n_groups - 1) / n_groups;`
    `const int64_t by_tiles = (n_tiles + n_waves - 1) / n_waves;`  `if (bpg > by_tiles) bpg = by_tiles;`
    `const int64_t stride = (int64_t)a.blocks_per_group * NW;`"""
    qg = min(qb, PQ_SCAN_KIB // M)
    n_groups = ceil_div(qb, qg)
    n_tiles, nw = ceil_div(n_docs, 64), pq_scan_threads(pieces(M)) // 64
    bpg = max(1, min(ceil_div(2 * max(cus, 1), n_groups), ceil_div(n_tiles, nw)))
    return qg, n_groups, bpg, bpg * nw, n_tiles


def pq_walks(qb, n_docs, M, cus):
    """Per workgroup of a query group, the tiles each of its waves walks: `int64_t t = (int64_t)r * NW + wave;` then `t + stride`
    while `t < a.n_tiles`."""
    _, _, bpg, stride, n_tiles = pq_scan_plan(qb, n_docs, M, cus)
    nw = stride // bpg
    return [[len(range(r * nw + w, n_tiles, stride)) for w in range(nw)] for r in range(bpg)]


def deep(walks):
    """The double buffer turns over (`step(b0, b1)`, `step(b1, b0)`, `step(b0, b1)`) and ends on both buffers: in one workgroup a
    wave walks at least 3 tiles and another one fewer."""
    return any(max(w) >= 3 and max(w) - 1 in w for w in walks)


# (dsub, dim, n): tests/test_pq_gpu.py's test_bit_for_bit at M = 40, 72, 90, 100 -> NP = 3, 5, 6, 7.  317 = 39 * 8 + 5 is a ragged
# last subspace, M = 100 leaves the last piece of NP = 7 partly empty.
PQ_INSTANCE_CASES = [(dsub, dim, n) for dsub, dim in ((8, 317), (4, 288), (8, 720), (8, 800)) for n in (1, 193)]
# (dsub, dim, n, nq): rows rebuilt from chosen codes.  M = 128 (NP = 8, 8 waves) and M = 112 (NP = 7, 16 waves) give one query per
# group, and 640 groups >= 2 * CUs up to 320 CUs, so blocks_per_group = 1: 28 and 55 tiles, the last one partial.
PQ_DEEP_CASES = [(4, 512, 27 * 64 + 37, 640), (8, 896, 54 * 64 + 21, 640)]
# (dsub, dim, n, nq): two passes of the query loop
PQ_PASS_CASES = [(16, 64, 193, PASS + 7)]
# (dsub, dim, n, m): srx_pq_score_docs past one trip and past one workgroup per query
PQ_SCORER_CASES = [(8, 200, 193, 1025), (8, 200, 193, 8192 + 5)]

# what tests/test_pq_gpu.py runs already: (dsub, dim, n, nq), and the m of its scorer calls
PQ_EXISTING = ([(dsub, dim, n, 33) for dsub in (4, 8, 16) for dim in (3, 200, 512, 1024) if ceil_div(dim, dsub) <= 128 for n in (1, 193)]  # test_bit_for_bit
               + [(16, 64, 40_000, 70),  # test_split_rows_and_query_groups
                  (8, 72, 193, 5),       # test_screen_that_covers_the_corpus_is_the_exact_search
                  (8, 48, 30, 1), (4, 48, 30, 1)])  # test_service: a few dozen docs, one query at a time
PQ_EXISTING_SCORER_M = [37, 193, 1, 7]


# =================================================================================================== dense_ivf.hip
IVF_TYPES = ("f16", "bf16")
IVF_DIM = 64  # of the probe and search cases


def ivf_plan(nq, nlist, nprobe, max_list_tiles):
    """(P, ldc, strip_bytes) of ivf_plan: `p.ldc = (int64_t)((nlist + 31) / 32) * 32;`  `p.strip_bytes = max_list_tiles * 128;`
    `int64_t qb = (1ll << 30) / ((int64_t)nprobe * p.strip_bytes);`  `qb = qb < 1 ? 1 : qb > IVF_PASS ? IVF_PASS : qb;`"""
    strip = max_list_tiles * 128
    return min(nq, max(1, min(PASS, (1 << 30) // (nprobe * strip)))), ceil_div(nlist, 32) * 32, strip


def ivf_workspace_bytes(nq, nlist, nprobe, k, max_list_tiles):
    """ivf_ws: the centroid scores of a pass, four [P * nprobe] arrays, four [nlist + 1] arrays, the strips, the lists of k, the merge"""
    P, ldc, strip = ivf_plan(nq, nlist, nprobe, max_list_tiles)
    N = P * nprobe
    return (r256(min(nq, PASS) * ldc * 4) + 4 * r256(N * 4) + 4 * r256((nlist + 1) * 4) + r256(N * strip) + 2 * r256(N * k * 4) + r256(N * 4)
            + merge_bytes(P, nprobe, k) + 256)


def ivf_passes(nq, P):
    """`for (int q0 = 0; q0 < nq; q0 += pl.P)` of srx_ivf_search; srx_ivf_probe steps by IVF_PASS"""
    return ceil_div(nq, P)


def ivf_centroid_slices(qb, nlist):
    """[centroid tiles of every blockIdx.y] of srx_ivf_centroid_scores_kernel:
    `const int qblocks = (nq + 31) / 32, n_ct = (nlist + 31) / 32;`  `int slices = 512 / qblocks < n_ct / 4 ? 512 / qblocks : n_ct / 4;`
    `n_ct * blockIdx.y / gridDim.y, n_ct * (blockIdx.y + 1) / gridDim.y`"""
    qblocks, n_ct = ceil_div(qb, 32), ceil_div(nlist, 32)
    s = max(1, min(512 // qblocks, n_ct // 4))
    return [n_ct * (y + 1) // s - n_ct * y // s for y in range(s)]


def ivf_select_trips(nlist, nprobe):
    """(chunks of the tie loop `for (int c0 = 0; c0 < nlist; c0 += THREADS)`, trips of the ranking loop
    `for (int i = tid; i < cnt; i += THREADS)` with cnt = min(nprobe, nlist)) of srx_ivf_probe_select_kernel"""
    return ceil_div(nlist, 256), ceil_div(min(nprobe, nlist), 256)


def ivf_crafted_scores(nlist):
    """The centroid scores of query 0 of every probe case (the query is a unit vector, the scores are column 0 of the centroids):
    three values, each of them in every 256-chunk of the lists."""
    return [1 if c % 11 == 5 else -1 if c % 4 == 1 else 0 for c in range(nlist)]


def ivf_select_ties(scores, nprobe):
    """(T, need, [keys == T per 256-chunk], [of them taken per chunk]) of the selection over one score row: T the kk-th largest,
    `need` of the keys equal to T are taken, lowest lists first."""
    kk = min(nprobe, len(scores))
    T = sorted(scores, reverse=True)[kk - 1]
    need = kk - sum(1 for s in scores if s > T)
    ties, taken, before = [], [], 0
    for c0 in range(0, len(scores), 256):
        t = sum(1 for s in scores[c0: c0 + 256] if s == T)
        ties.append(t)
        taken.append(max(0, min(t, need - before)))
        before += t
    return T, need, ties, taken


def ivf_scan_slices(qb, nprobe, nlist):
    """gridDim.y of srx_ivf_scan_kernel: `groups_max = (d.nlist < n_pairs ? d.nlist : n_pairs) + n_pairs / 32`,
    `slices = 1024u / groups_max < 1u ? 1u : 1024u / groups_max > 16u ? 16u : 1024u / groups_max`"""
    n_pairs = qb * nprobe
    return max(1, min(16, 1024 // (min(nlist, n_pairs) + n_pairs // 32)))


def ivf_rank_trips(list_size):
    """Trips of `for (int64_t c0 = 0; c0 < cols; c0 += THREADS * IVF_NPT)` over a list's strip: cols = 32-row tiles * 32, 1024 a trip"""
    return ceil_div(ceil_div(list_size, 32) * 32, 1024)


def ivf_update_rounds(members):
    """(rounds, chunks of the last round) of srx_ivf_update_kernel: `round0 += (int64_t)WAVES * IVF_CHUNK` (4 * 256 members); a chunk
    exists while `round0 + (int64_t)w * IVF_CHUNK < m1`"""
    rounds = ceil_div(members, 1024)
    return rounds, ceil_div(members - (rounds - 1) * 1024, 256) if members else 0


def ivf_assign_vec(dim, ld, base_offset):
    """`const bool vec = ((uintptr_t)rows & 15) == 0 && ld % 4 == 0 && dim % 4 == 0;` with the base `base_offset` floats past a
    16-byte boundary"""
    return base_offset % 4 == 0 and ld % 4 == 0 and dim % 4 == 0


# (nlist, nprobe, nq, dtype): integer centroids and queries in {-1, 0, 1}; query 0 is the crafted row
IVF_PROBE_CASES = [(nlist, nprobe, nq, dtype) for nlist, dtype, probes in ((257, "f16", (1, 256, 257)), (1024, "bf16", (257, 1000, 1024)),
                                                                            (1500, "f16", (1, 256, 1000, 1024)))
                   for nprobe in probes for nq in (1, 33)]
# (nlist, nprobe, nq, dtype): two passes of srx_ivf_probe
IVF_PROBE_PASS_CASES = [(257, 3, PASS + 3, "f16")]
# the lists of the search cases: one of 66 tiles (3 rank trips) beside an empty one, 1 row and 31 / 32 / 33 rows
IVF_SEARCH_SIZES = (33, 0, 2100, 1, 31, 32)
# (dtype, nq, nprobe, k): plain, filtered, offset and a given probe_list each
IVF_SEARCH_CASES = [(dtype, nq, nprobe, k) for dtype in IVF_TYPES for nq, nprobe, k in ((1, 1, 1024), (1, 6, 10), (33, 2, 1), (33, 3, 10), (33, 6, 1024))]
# (dtype, nq, nprobe, k): two passes of srx_ivf_search
IVF_SEARCH_PASS_CASES = [("f16", PASS + 5, 2, 10)]
# (dtype, dim, ld, base_offset): 130 centroids, 100 rows; dim 30 and 201 are no multiples of 4, (64, 67, 0) is a row stride that is
# none, (64, 68, 1) a base 4 bytes past a 16-byte boundary; (64, 68, 0) is a strided view that still loads 16 bytes
IVF_ASSIGN_NLIST, IVF_ASSIGN_ROWS = 130, 100
IVF_ASSIGN_CASES = [(dtype, dim, ld, off) for dtype in IVF_TYPES for dim, ld, off in ((30, 30, 0), (201, 201, 0), (64, 67, 0), (64, 68, 1), (64, 68, 0))]
# the members per list of the update cases, and their (dim,)
IVF_UPDATE_LENS = (0, 1, 255, 256, 257, 513, 0, 5, 1023, 1024, 1025, 2305)
IVF_UPDATE_CASES = [(1,), (64,), (65,), (200,)]

# what tests/test_ivf_gpu.py and tests/test_ivfpq_gpu.py run already
IVF_EXISTING_NLIST = [1, 3, 33, 130, 20, 8, 6, 7, 5, 4]  # every probe select and centroid-score launch: nlist <= 130
IVF_EXISTING_MAX_NQ = 129
IVF_EXISTING_MAX_LIST = 140                  # rows of the longest list a search ranks (test_integers_bit_for_bit's SIZES)
IVF_EXISTING_UPDATE_LENS = (0, 1, 255, 256, 257, 513, 0, 5)  # before this table extended them
IVF_EXISTING_ASSIGN = [(dtype, dim, True) for dtype in IVF_TYPES for dim in (64, 200, 768)] + [("bf16", 40, True)]  # (dtype, dim, vec) against a reference


# =================================================================================================== dense_ivfpq.hip
def ivfpq_scan_threads(np_):
    """`constexpr int ivfpq_scan_threads(int np) { return np <= 2 ? 256 : (np == 6 || np == 7) ? 1024 : 512; }`"""
    return 256 if np_ <= 2 else 1024 if np_ in (6, 7) else 512


def ivfpq_plan(nq, nlist, nprobe, max_list_tiles):
    """(P, S, L) of ivfpq_plan: `const int64_t T = (int64_t)nprobe * max_list_tiles;`  `int64_t qb = (1ll << 30) / (256 * T);`
    `qb = qb < 1 ? 1 : qb > IVFPQ_PASS ? IVFPQ_PASS : qb;`  `int64_t s = 512 / (p.P > 0 ? p.P : 1);`  `if (s > 64) s = 64;`
    `if (s > (T + 15) / 16) s = (T + 15) / 16;`  `p.L = (T + p.S - 1) / p.S;`"""
    T = nprobe * max_list_tiles
    P = min(nq, max(1, min(PASS, (1 << 30) // (256 * T))))
    S = max(1, min(512 // max(P, 1), 64, (T + 15) // 16))
    return P, S, ceil_div(T, S)


def ivfpq_workspace_bytes(nq, nlist, nprobe, k, M, max_list_tiles):
    """ivfpq_ws: centroid scores, tables, four [P * nprobe] arrays, pre, the strips and their tiles, the lists of k, the merge"""
    P, S, L = ivfpq_plan(nq, nlist, nprobe, max_list_tiles)
    N, items = P * nprobe, P * S
    return (r256(P * ceil_div(nlist, 32) * 32 * 4) + r256(P * M * 1024) + 4 * r256(N * 4) + r256(P * (nprobe + 1) * 4) + r256(items * L * 256)
            + r256(items * L * 4) + 2 * r256(items * k * 4) + r256(items * 4) + merge_bytes(P, S, k) + 256)


def ivfpq_list_tiles(sizes):
    return [ceil_div(s, 64) for s in sizes]


def ivfpq_walks(sizes, probed, S, np_):
    """Per slice of a query that reads the lists `probed` (in slot order, distinct): (the tiles each wave of the workgroup walks,
    the list boundaries a wave crosses at most, the slice's columns for the rank kernel).  ivfpq_slice:
    `const int per = (total + S - 1) / S;`  `g0 = min(s * per, total);`  `g1 = min(g0 + per, total);`; the scan: `int g = g0 + wave;`
    then `g + NW` while `g < g1`."""
    tiles = ivfpq_list_tiles(sizes)
    slot_of = [j for j, c in enumerate(probed) for _ in range(tiles[c])]  # the slot of every tile of the concatenation
    total, nw = len(slot_of), ivfpq_scan_threads(np_) // 64
    per = ceil_div(total, S)
    out = []
    for s in range(S):
        g0 = min(s * per, total)
        g1 = min(g0 + per, total)
        walks = [list(range(g0 + w, g1, nw)) for w in range(nw)]
        crossed = max((len({slot_of[g] for g in w}) - 1 for w in walks if w), default=0)
        out.append(([len(w) for w in walks], crossed, (g1 - g0) * 64))
    return out


def ivfpq_rank_trips(cols):
    """Trips of `for (int64_t c0 = 0; c0 < cols; c0 += THREADS * IVFPQ_NPT)`"""
    return ceil_div(cols, 1024)


def ivfpq_prepare(nprobe):
    """(trips of the `j += THREADS` loops, threads that own slots in the prefix, the thread that writes pre[nprobe]) of
    srx_ivfpq_prepare_kernel: thread t owns slots 4 t .. 4 t + 3; `if (4 * tid < a.nprobe && 4 * tid + 4 >= a.nprobe)`"""
    owners = [t for t in range(256) if 4 * t < nprobe <= 4 * t + 4]
    assert len(owners) == 1
    return ceil_div(nprobe, 256), ceil_div(nprobe, 4), owners[0]


IVFPQ_SIZES = (0, 1, 63, 64, 65, 200)  # tests/test_ivfpq_gpu.py's SIZES: what the instance, pass and scorer cases use
# (dsub, dim, dtype): test_ivfpq_gpu.py's test_bit_for_bit at M = 40, 72, 100, 128 -> NP = 3, 5, 7, 8; (16, f16) and (4, bf16) are
# the two encoder instances its SHAPES leave out
IVFPQ_INSTANCE_CASES = [(16, 637, "f16"), (4, 288, "bf16"), (8, 800, "f16"), (8, 1024, "bf16")]
# lists of 25 tiles beside an empty one and short ones: 53 tiles in all, one slice (S = 1) for more than 512 queries
IVFPQ_DEEP_SIZES = (1600, 0, 70, 1, 1540)
# (dsub, dim, dtype, nq): rows rebuilt from chosen codes; NP = 7 (16 waves), NP = 8 (8 waves), NP = 1 (4 waves)
IVFPQ_DEEP_CASES = [(8, 896, "f16", 513), (8, 1024, "bf16", 513), (4, 64, "f16", 513)]
# (dsub, dim, dtype, nq, nprobe): two passes, the engine's probe and a given probe_list
IVFPQ_PASS_CASES = [(4, 8, "f16", PASS + 9, 3)]
# (nprobe,): 1024 lists of 0, 1, 2 rows (c % 3) and a few of 65 (c % 97 == 0); dsub 4, dim 16, three queries
IVFPQ_PREPARE_NLIST = 1024
IVFPQ_PREPARE_CASES = [(255,), (257,), (1023,), (1024,)]
# (dsub, dim, dtype, m): srx_ivfpq_score_docs past one trip and past one workgroup per query
IVFPQ_SCORER_CASES = [(8, 200, "bf16", 1025), (8, 200, "bf16", 8192 + 5)]


def ivfpq_prepare_sizes():
    return [65 if c % 97 == 0 else c % 3 for c in range(IVFPQ_PREPARE_NLIST)]


# what tests/test_ivfpq_gpu.py runs already
IVFPQ_EXISTING = [(4, 3, "f16"), (8, 200, "bf16"), (8, 768, "f16"), (16, 1024, "bf16"),  # test_bit_for_bit (SHAPES), lists of IVFPQ_SIZES
                  (4, 8, "f16"),      # test_slices_cut_lists
                  (8, 40, "bf16"),    # test_assignment
                  (8, 30, "f16"),     # test_training
                  (8, 72, "f16"),     # test_screen_that_covers_the_corpus_is_the_exact_search
                  (8, 48, "f16"), (4, 48, "f16")]  # test_service
IVFPQ_EXISTING_SLICED = ((3, 40 * 64 + 5, 70), 4, 1, 3)  # test_slices_cut_lists: (sizes, dsub -> M = 2, nq, nprobe): its deepest walk
IVFPQ_EXISTING_MAX_NQ, IVFPQ_EXISTING_MAX_NPROBE = 33, 6
IVFPQ_EXISTING_SCORER_M = [37, 384, 2]
