"""The dense family's kernel instances and loop shapes as a table: per unit (dense_half.hip, maxsim.hip, mmr.hip,
dense_binary.hip, dense_score.hip, dense_quant.hip) the dispatch rule of the host side restated in Python, the GPU cases of
tests/test_dense_instances_gpu.py as plain tuples, and the shapes the unit's own test file already runs.  A plain module, as
the ``*_ref.py`` files are: it never imports the package.  tests/test_dense_instances_cpu.py parses the dispatch lines of the
kernel sources and asserts that these cases and the existing shapes together reach every instantiated kernel and every loop
shape named there; the GPU file parametrizes over these lists and over nothing else, so the two cannot drift apart.

A new instance on a dispatch line needs a case here before the CPU test passes again."""

BASE = 7_000_000  # the doc_base of the cases that have one


def pad64(dim):
    return (dim + 63) // 64 * 64


def pad128(dim):
    return (dim + 127) // 128 * 128


# =================================================================================================== dense_half.hip
HALF_TYPES = ("f16", "bf16")
HALF_QTILE = 128   # HF_QTILE: queries per workgroup of the GEMM
HALF_PASS = 1024   # the cap of half_plan's QB: queries per pass
HALF_KB = 4        # HG_KB: k-steps (of 16 columns) per stage of the GEMM's K loop


def half_convert_instance(dim, ld=None, aligned=True):
    """(NJ, VEC) of srx_dense_half_convert_kernel: nj = (dim_pad + 255) / 256; 16-byte loads iff the base is 16-byte
    aligned and ld and dim are multiples of 4."""
    ld = dim if ld is None else ld
    return -(-pad64(dim) // 256), bool(aligned and ld % 4 == 0 and dim % 4 == 0)


def half_n_stages(dim):
    """Trips of the GEMM's K loop: ks / HG_KB with ks = dim_pad / 16."""
    return pad64(dim) // 16 // HALF_KB


def half_passes(nq, n_docs):
    """(query passes, query tiles of the largest pass) of srx_dense_search_half (half_plan: QB in 32 .. 1024)."""
    ld = pad64(n_docs)
    qb = min(max((4 << 30) // (ld * 4) // 32 * 32, 32), HALF_PASS)
    return -(-nq // qb), -(-min(nq, qb) // HALF_QTILE)


# (dim, n): conversion bytes.  257 and 383: NJ = 2 with scalar loads; 320, 384, 512: NJ = 2 with 16-byte loads; 705 and 961: the
# scalar-load form of NJ = 3 and NJ = 4 (test_half_gpu.py converts 768, 1000 and 1024 only: multiples of 4)
HALF_CONVERT_CASES = [(dim, n) for dim in (257, 320, 383, 384, 512, 705, 961) for n in (33, 100)]
# (n, nq, dim, k): integers in [-3, 3]; n_stages 3, 5, 6, 7, 9, 13, 15
HALF_INT_CASES = ([(129, 33, dim, k) for dim in (192, 320, 321, 448, 576, 832, 960) for k in (10, 1024)]
                  + [(4099, 129, dim, k) for dim in (192, 960) for k in (10, 1024)])
# (n, dim): random normal rows, 33 queries
HALF_RANDOM_CASES = [(4099, 320)]
# (n, dim, nq, k, n_rows): a filter of n_rows disjoint residue rows, q_filter[i] = i % (n_rows + 1) - 1; two passes, nine query tiles
HALF_FILTER_CASES = [(200, 64, 1030, 10, 4)]

# what tests/test_half_gpu.py runs already
HALF_EXISTING_CONVERT = [  # (dim, ld, base 16-byte aligned)
    (1, 1, True), (3, 3, True), (63, 63, True), (64, 64, True), (65, 65, True), (200, 200, True), (768, 768, True), (1000, 1000, True),
    (1024, 1024, True),   # test_convert_every_row_length
    (200, 203, False),    # test_convert_slice_chunks_junk_and_stream: a column slice, the base 4 bytes off
    (65, 65, True),       # test_convert_non_finite_rows
]
HALF_EXISTING_SEARCH_DIMS = [1, 64, 65, 1024,  # test_exact_on_small_integers (INT_CASES)
                             128, 200, 768]    # test_search_is_the_ranking_of_the_scorers_bits (SHAPES)
HALF_EXISTING_FILTERED = [(32801, 33, True),     # (n, nq, filtered) test_filtered_search
                          (4099, 1025, False)]   # test_exact_on_small_integers: the only second pass, unfiltered


# =================================================================================================== maxsim.hip
MAXSIM_G = 4  # MS_G: k-steps per group of B loads


def maxsim_nab(tq):
    """NAB of srx_maxsim_score_kernel: blocks of 32 query tokens."""
    return -(-tq // 32)


def maxsim_gpb(dim):
    """Groups of B loads per block of 32 doc tokens: ks / MS_G."""
    return pad64(dim) // 16 // MAXSIM_G


def maxsim_shape_ok(tq, dim):
    return 1 <= tq <= 128 and maxsim_nab(tq) * 32 * pad64(dim) <= 32768


# (dim, tq): the score form, nq = 3, m = 40
MAXSIM_CASES = [(64, 65), (64, 96), (192, 33), (192, 96), (192, 128), (320, 1), (320, 65)]
# (dim, tq, m, k): the rerank form
MAXSIM_RERANK_CASES = [(192, 96, 65, 65)]

# what tests/test_late_gpu.py runs already: (dim, tq)
MAXSIM_EXISTING = [(48, 1), (48, 31), (48, 32), (48, 33), (128, 1), (128, 31), (128, 32), (128, 33), (1024, 1), (1024, 31), (1024, 32),
                   (500, 64), (256, 128),  # test_exact_integers (SHAPES)
                   (128, 33),              # test_every_similarity_negative, test_degenerate_inputs
                   (96, 33), (96, 20),     # test_bits_of_the_existing_scorer_and_fp64_bound, test_bits_do_not_depend_on_the_batch
                   (48, 9), (48, 6)]       # test_candidate_list_edges, test_rerank


# =================================================================================================== mmr.hip
MMR_PIECES = 2048  # MG_PIECES: 16-byte pieces of one K chunk in LDS
MMR_WAVES = 16     # MG_WAVES: a wave owns TPW tiles of 32 x 32
MMR_F32_BUCKETS = (1, 2, 4, 8, 12, 16)


def mmr_half_plan(dim, m):
    """(nb, kc, TPW, chunk list, tiles) of srx_mmr_gram_half_kernel: nb blocks of 32 positions, kc k-steps per chunk, the
    lengths of the K chunks in order, nb * nb tiles over 16 * TPW tile slots."""
    nb, ks = -(-m // 32), pad64(dim) // 16
    kc = MMR_PIECES // (nb * 64)
    return nb, kc, (1 if m <= 128 else 4), [min(kc, ks - c0) for c0 in range(0, ks, kc)], nb * nb


def bucket(ns, buckets):
    """The first bucket >= ns: the `if (ns <= NS)` ladders of mmr.hip and dense_score.hip."""
    return next(b for b in buckets if b >= ns)


def mmr_f32_ns(dim):
    """(NS of srx_mmr_gram_f32_kernel, whether the bucket is wider than the row)"""
    ns = pad64(dim) // 64
    b = bucket(ns, MMR_F32_BUCKETS)
    return b, b > ns


# (dim, m): bits of the scorer + the restatement; nq = 5, k = min(10, m)
MMR_HALF_CASES = [(200, m) for m in (65, 96, 129, 160, 161, 192, 193, 224)] + [(768, 32)]
MMR_HALF_EXACT_CASES = [(200, 96), (200, 160)]  # small integers against gram_exact / select_naive_f64
MMR_F32_CASES = [(dim, 100) for dim in (192, 320, 512, 576, 832)]
MMR_F32_EXACT_CASES = [(320, 100)]

# what tests/test_mmr_gpu.py runs already: (dim, m), f32 and both half types alike unless said
MMR_EXISTING = [(200, 100), (200, 1), (200, 31), (200, 32), (200, 33), (200, 256), (64, 100), (768, 100), (1024, 100),
                (1024, 256),             # test_bits_against_the_scorer_and_the_restatement (CASES)
                (200, 100), (1024, 33),  # test_small_integers_are_exact
                (200, 40),               # test_edges
                (768, 100),              # test_a_row_does_not_depend_on_the_batch
                (96, 30)]                # test_service_diversify_and_hybrid (f32 and f16): lists of at most 30 docs
MMR_EXISTING_HALF_ONLY = [(64, 33)]      # test_large_batch_is_split (f16)


# =================================================================================================== dense_binary.hip
BINARY_QTILE = 128  # BN_QTILE
BINARY_PASS = 1024  # BN_PASS


def binary_nj(dim):
    """NJ of srx_binary_dist_kernel and nj of srx_binary_dist_docs: 16-byte pieces per doc, dim_pad / 128."""
    return pad128(dim) // 128


def binary_passes(nq, n_docs):
    """(query passes, query tiles of the largest pass) of srx_binary_search (bin_plan: QB in 32 .. 1024)."""
    ld = (n_docs + 63) // 64 * 64
    qb = min(max((4 << 30) // (ld * 2) // 32 * 32, 32), BINARY_PASS)
    return -(-nq // qb), -(-min(nq, qb) // BINARY_QTILE)


# (dim, n, m, doc_base) with nq = 3; one filtered call and the encoder per dim
BINARY_SEARCH_CASES = [(dim, n, m, base) for dim in (129, 257, 384, 400, 513, 640, 700, 768, 896, 1000) for n in (65, 200) for m in (1, 70)
                       for base in (0, BASE)]
# (dim,): hamming_docs, one dim per nj = 1 .. 8
BINARY_DOCS_CASES = [(100,), (200,), (300,), (500,), (600,), (700,), (800,), (1000,)]
# (n, dim, nq, m, n_rows): as HALF_FILTER_CASES
BINARY_FILTER_CASES = [(200, 96, 1030, 16, 4)]

# what tests/test_binary_gpu.py runs already
BINARY_EXISTING_SEARCH_DIMS = [32,    # test_search_at_every_size_edge, test_search_massive_ties_across_chunks_and_splits
                               40,    # test_search_m_edges_and_merge_capacity
                               70,    # test_search_query_counts
                               1024,  # test_search_dim_1024_complement_and_doc_base
                               96,    # test_filtered_search_rows_and_q_filter
                               200]   # test_dist_docs_equals_the_search_and_the_restatement
BINARY_EXISTING_DOCS_DIMS = [200]     # test_dist_docs_equals_the_search_and_the_restatement
BINARY_EXISTING_FILTERED = [(200, 8, True),      # (n, nq, filtered) test_filtered_search_rows_and_q_filter
                            (300, 1025, False)]  # test_search_query_counts: the only second pass, unfiltered


# =================================================================================================== dense_score.hip
SCORE_BUCKETS = ((1, 8), (2, 8), (4, 8), (8, 8), (16, 4))  # (NS, U) of srx_dense_score_rows_kernel
SCORE_I8_DIMS = (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024)
SCORE_I8_LADDER = {1: 2, 2: 4, "else": 8}  # glog -> U of srx_dense_score_i8_kernel


def score_rows_instance(dim):
    """((NS, U), slack) of srx_dense_score_rows_kernel for f32 and u8 rows alike: the first bucket >= dim / 64."""
    ns = dim // 64
    b = next(p for p in SCORE_BUCKETS if p[0] >= ns)
    return b, b[0] > ns


def score_i8_glog(dim):
    """log2 of the lanes that share a candidate: the next power of two >= dim / 16 pieces."""
    g = 0
    while (1 << g) < dim // 16:
        g += 1
    return g


def score_i8_u(dim):
    g = score_i8_glog(dim)
    return SCORE_I8_LADDER.get(g, SCORE_I8_LADDER["else"])


SCORE_SHAPES = [(65, 257), (64, 5), (1, 1)]  # (m, nq) of every scorer case
# (engine, dim, n_docs)
SCORE_ROWS_CASES = [(engine, dim, 1000) for engine in ("f32", "u8") for dim in (256, 320, 512, 832)]
# (dim, n_docs, packed)
SCORE_I8_CASES = [(dim, 1000, packed) for dim in (256, 384, 512) for packed in (True, False)]

# what tests/test_rescore_gpu.py compares with tests/rescore_ref.py already: (engine, dim)
SCORE_EXISTING_ROWS = [("f32", 64), ("f32", 128), ("f32", 1024), ("u8", 64), ("u8", 128), ("u8", 1024),  # test_dense_score_rows_kernels
                       ("f32", 192), ("u8", 64)]  # test_dense_score_doc_base_null_count_and_out_reuse
SCORE_EXISTING_I8_DIMS = [32, 96, 768, 1024,  # test_dense_score_i8_kernel
                          192, 64]            # test_dense_score_doc_base_null_count_and_out_reuse


# =================================================================================================== dense_quant.hip
QUANT_MODES = ("i8 rows", "i8 queries", "u8 rows", "u8 queries")  # DQ_I8_ROW, DQ_I8_QUERY, DQ_U8_ROW, DQ_U8_QUERY
QUANT_I8_DIMS = (32, 64, 96, 128, 192, 256, 384, 512, 768, 1024)


def quant_pads(dim):
    """(dim_pad of the i8 forms, dim_pad of the u8 forms)"""
    return next(d for d in QUANT_I8_DIMS if d >= dim), pad64(dim)


def quant_instances(dim):
    """The (NJ, VEC, mode) instances of srx_dense_quant_kernel the views of tests/test_quant_gpu.py reach at a row length:
    ``dense`` and ``wide`` load 16 bytes when dim % 4 == 0, ``slice`` never does; all four modes run on every view."""
    pi, pu = quant_pads(dim)
    vecs = {False} | ({True} if dim % 4 == 0 else set())
    return {(-(-pad // 256), v, mode) for mode in QUANT_MODES for pad in ((pi,) if mode.startswith("i8") else (pu,)) for v in vecs}


# (dim, n): all four modes, the packed and the row-major layout, every view
QUANT_CASES = [(dim, n) for dim in (257, 384, 512) for n in (33, 300)]
# what tests/test_quant_gpu.py runs already: test_bits_at_every_row_count_and_stride (DIMS).  No other test quantises on the
# device at a row length of 257 .. 512: test_dense_int8.py builds its dim-384 index from codes made on the host.
QUANT_EXISTING_DIMS = [1, 3, 31, 32, 33, 48, 63, 64, 65, 100, 768, 1000, 1024]
