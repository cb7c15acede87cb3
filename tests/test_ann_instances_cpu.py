"""The inventory of the kernel instances and loop shapes of dense_pq.hip, dense_ivf.hip and dense_ivfpq.hip, without a GPU.  The
dispatch lines are parsed (the SRX_PQ and SRX_IVFPQ lists, the `switch (dsub)` launches, the SRX_IVF_ASSIGN macro); the cases of
tests/ann_instances.py, together with the shapes the units' own test files run, must reach exactly the parsed sets.  The plan
rules the table restates are compared with the package's own formulas and with the library's workspace entry points, and every
loop shape the GPU file exists for must be reached by a case -- at 256 compute units and at a spread of other counts where the
plan depends on them.  An instance added to a dispatch line, or a case taken out of the table, fails here."""
import os
import re

import ann_instances as T
from sparse_rx import _capi, ivf, ivfpq, pq

MB = 1 << 20
TYPE_NAMES = {"SRX_HALF_F16": "f16", "SRX_HALF_BF16": "bf16"}


def _src(name):
    with open(os.path.join(_capi.CSRC_DIR, name), encoding="utf-8") as f:
        return f.read()


def _macro_args(src, macro):
    """The numbers of every use of a one-argument dispatch macro (its #define has a name, not a number, as argument)."""
    return [int(a) for a in re.findall(rf"\b{macro}\((\d+)\)", src)]


def _dsub_launches(src):
    """{(kernel, dsub)} of the `switch (dsub)` launches: `case 4: hipLaunchKernelGGL((kernel<4, ...` and the default."""
    found = re.findall(r"(?:case (\d+)|default): hipLaunchKernelGGL\(\(?(srx_\w+)<(\d+)", src)
    assert found and all(c in ("", d) for c, _, d in found)
    return {(kernel, int(d)) for _, kernel, d in found}


def _quoted(src, *lines):
    for line in lines:
        assert line in src, f"the source no longer holds `{line}`: restate the rule in tests/ann_instances.py"


def _unreached(unit, what, parsed, reached):
    """Both directions: an instance no case reaches, and a case whose instance the source no longer has."""
    parsed, reached = set(parsed), set(reached)
    assert parsed, f"{unit}: no {what} instance found in the source: the dispatch line has changed, update the parser"
    missing, gone = sorted(parsed - reached, key=repr), sorted(reached - parsed, key=repr)
    assert not missing, f"{unit}: no case of tests/ann_instances.py and no existing test reaches {what} {missing}"
    assert not gone, f"{unit}: the table reaches {what} {gone}, which the dispatch line does not instantiate"


def _has(unit, shape, found):
    assert found, f"{unit}: tests/ann_instances.py holds no case for the loop shape '{shape}'"


def _np(dsub, dim):
    return T.pieces(T.subspaces(dim, dsub))


# ---- dense_pq.hip ---------------------------------------------------------------------------------------------------------------
PQ_SEARCHES = T.PQ_INSTANCE_CASES + [c[:3] for c in T.PQ_DEEP_CASES + T.PQ_PASS_CASES + T.PQ_SCORER_CASES]


def test_pq_scan_and_dsub_instances():
    src = _src("dense_pq.hip")
    _quoted(src, "inline int pq_pieces(int M) { return (M + 15) / 16; }",
            "constexpr int pq_scan_threads(int np) { return np < 8 ? PQ_SCAN_THREADS : PQ_SCAN_THREADS / 2; }", "constexpr int PQ_SCAN_THREADS = 1024;",
            "switch (pq_pieces(a.M)) {", "*M = (dim + dsub - 1) / dsub;")
    parsed = _macro_args(src, "SRX_PQ")
    assert len(parsed) == len(set(parsed))
    old = {_np(dsub, dim) for dsub, dim, _, _ in T.PQ_EXISTING}
    new = {_np(dsub, dim) for dsub, dim, _ in T.PQ_INSTANCE_CASES}
    _unreached("dense_pq.hip", "srx_pq_scan_kernel NP", parsed, old | new)
    assert old == {1, 2, 4, 8} and new == {3, 5, 6, 7}  # the gap, and one bit-for-bit case per missing instance
    for np_ in new:  # at one row and at four tiles each
        assert {n for dsub, dim, n in T.PQ_INSTANCE_CASES if _np(dsub, dim) == np_} == {1, 193}
    Ms = {T.subspaces(dim, dsub) for dsub, dim, _ in T.PQ_INSTANCE_CASES}
    _has("dense_pq.hip", "a ragged last subspace", any(dim % dsub for dsub, dim, _ in T.PQ_INSTANCE_CASES))
    _has("dense_pq.hip", "NP = 7 with a partly empty last piece", any(T.pieces(M) == 7 and M % 16 for M in Ms))
    # the `switch (dsub)` launches: encoder (both layouts share the switch), table kernel and scorer
    launches = _dsub_launches(src)
    assert {k for k, _ in launches} == {"srx_pq_encode_kernel", "srx_pq_lut_kernel", "srx_pq_score_docs_kernel"}
    reached = {(k, dsub) for k in ("srx_pq_encode_kernel", "srx_pq_lut_kernel") for dsub, _, _ in PQ_SEARCHES}
    reached |= {("srx_pq_score_docs_kernel", dsub) for dsub, _, _ in T.PQ_INSTANCE_CASES + [c[:3] for c in T.PQ_SCORER_CASES]}
    reached |= {(k, dsub) for k, _ in launches for dsub, _, _, _ in T.PQ_EXISTING[:-4]}  # test_bit_for_bit runs all three
    _unreached("dense_pq.hip", "(kernel, dsub) launch", launches, reached)


def test_pq_loop_shapes():
    src = _src("dense_pq.hip")
    _quoted(src, "constexpr int PQ_SCAN_FLOATS = 144 * 256;", "const int qg_max = PQ_SCAN_FLOATS / (M * 256);",
            "const int qg = qb < qg_max ? qb : qg_max, n_groups = (qb + qg - 1) / qg;",
            "int64_t bpg = (2 * (int64_t)(n_cus > 0 ? n_cus : 1) + n_groups - 1) / n_groups;", "const int64_t by_tiles = (n_tiles + n_waves - 1) / n_waves;",
            "if (bpg > by_tiles) bpg = by_tiles;", "const int64_t stride = (int64_t)a.blocks_per_group * NW;", "int64_t t = (int64_t)r * NW + wave;",
            "for (int q0 = 0; q0 < nq; q0 += p.QB) {", "constexpr int PQ_DOCS_CHUNK = 8 * PQ_SCAN_THREADS;",
            "const dim3 grid((unsigned)nq, (unsigned)(chunks < 64 ? chunks : 64));", "q_filter[q0 + q]")
    # the double buffer: no wave of an existing test walks a second tile; the deep cases turn it over at every CU count
    for dsub, dim, n, nq in T.PQ_EXISTING:
        for qb in T.pq_passes(nq, n):
            assert max(max(w) for w in T.pq_walks(qb, n, T.subspaces(dim, dsub), T.CUS)) <= 1, (dsub, dim, n, nq)
    for dsub, dim, n, nq in T.PQ_DEEP_CASES:
        M = T.subspaces(dim, dsub)
        assert n % 64 != 0 and T.pq_passes(nq, n) == [nq] and T.pq_workspace_bytes(nq, n, M, 1024) < 100 * MB
        for cus in (T.CUS,) + T.CU_SPREAD:
            qg, n_groups, bpg, stride, n_tiles = T.pq_scan_plan(nq, n, M, cus)
            assert (qg, bpg) == (1, 1) and n_groups >= 2 * cus, (M, cus)  # no dependence on the CU count
            walks = T.pq_walks(nq, n, M, cus)
            assert T.deep(walks) and sorted(set(walks[0])) == [3, 4], (M, cus, walks)
    deep = {_np(dsub, dim) for dsub, dim, _, _ in T.PQ_DEEP_CASES}
    assert deep == {7, 8} and {T.pq_scan_threads(np_) for np_ in deep} == {1024, 512}
    # the pass loop
    assert all(len(T.pq_passes(nq, n)) == 1 for _, _, n, nq in T.PQ_EXISTING)
    _has("dense_pq.hip", "a second pass", any(len(T.pq_passes(nq, n)) >= 2 for _, _, n, nq in T.PQ_PASS_CASES))
    assert T.PASS % 3 != 0  # a q_filter of period 3 reads other rows behind the pass boundary
    # the scorer of given docs
    assert {T.scorer_grid(m) for m in T.PQ_EXISTING_SCORER_M} == {(1, 1)}
    grids = {T.scorer_grid(m) for _, _, _, m in T.PQ_SCORER_CASES}
    _has("dense_pq.hip", "a scorer thread with two trips", any(gy == 1 and trips >= 2 for gy, trips in grids))
    _has("dense_pq.hip", "a scorer gridDim.y of two", any(gy >= 2 and trips >= 2 for gy, trips in grids))
    assert grids == {(1, 2), (2, 5)}


# ---- dense_ivf.hip --------------------------------------------------------------------------------------------------------------
def test_ivf_assign_instances():
    src = _src("dense_ivf.hip")
    _quoted(src, "const bool vec = ((uintptr_t)rows & 15) == 0 && ld % 4 == 0 && dim % 4 == 0;", "#define SRX_IVF_ASSIGN(T)")
    types = [TYPE_NAMES[t] for t in re.findall(r"SRX_IVF_ASSIGN\((SRX_HALF_\w+)\)", src)]
    forms = re.findall(r"hipLaunchKernelGGL\(\(srx_ivf_assign_kernel<T, (true|false)>\)", src)
    assert sorted(types) == ["bf16", "f16"] and sorted(forms) == ["false", "true"]
    parsed = {(t, f == "true") for t in types for f in forms}
    new = {(dtype, T.ivf_assign_vec(dim, ld, off)) for dtype, dim, ld, off in T.IVF_ASSIGN_CASES}
    old = {(dtype, vec) for dtype, _, vec in T.IVF_EXISTING_ASSIGN}
    _unreached("dense_ivf.hip", "srx_ivf_assign_kernel (TYPE, VEC)", parsed, new | old)
    assert not any(not vec for _, vec in old) and {(t, False) for t in T.IVF_TYPES} <= new  # the gap: no scalar-load form against a reference
    for dtype in T.IVF_TYPES:  # each way to lose the 16-byte loads, and a strided view that keeps them
        mine = [(dim, ld, off) for d, dim, ld, off in T.IVF_ASSIGN_CASES if d == dtype]
        assert any(dim % 4 for dim, _, _ in mine) and any(dim % 4 == 0 and ld % 4 for dim, ld, _ in mine)
        assert any(dim % 4 == 0 and ld % 4 == 0 and off % 4 for dim, ld, off in mine) and any(ld > dim and T.ivf_assign_vec(dim, ld, off) for dim, ld, off in mine)
        assert {dim for dim, _, _ in mine} >= {30, 201}
    assert T.IVF_ASSIGN_NLIST > 128  # a wave of the walk takes a second centroid tile


def test_ivf_loop_shapes():
    src = _src("dense_ivf.hip")
    _quoted(src, "constexpr int IVF_MAX_LIST = 65536, IVF_MAX_PROBE = 1024, IVF_PASS = 1024;", "constexpr int IVF_CHUNK = 256;", "constexpr int IVF_NPT = 4;",
            "for (int c0 = 0; c0 < nlist; c0 += THREADS) {", "for (int i = tid; i < cnt; i += THREADS) {",
            "const int qblocks = (nq + 31) / 32, n_ct = (nlist + 31) / 32;", "int slices = 512 / qblocks < n_ct / 4 ? 512 / qblocks : n_ct / 4;",
            "n_ct * blockIdx.y / gridDim.y, n_ct * (blockIdx.y + 1) / gridDim.y",
            "for (int64_t round0 = m0; round0 < m1; round0 += (int64_t)WAVES * IVF_CHUNK) {", "if (round0 + (int64_t)w * IVF_CHUNK < m1)",
            "for (int64_t c0 = 0; c0 < cols; c0 += THREADS * IVF_NPT) {", "int64_t qb = (1ll << 30) / ((int64_t)nprobe * p.strip_bytes);",
            "for (int q0 = 0; q0 < nq; q0 += pl.P) {", "for (int q0 = 0; q0 < nq; q0 += IVF_PASS) {", "p.strip_bytes = max_list_tiles * 128;")
    assert _capi.SRX_IVF_PASS == T.PASS == _capi.SRX_IVF_MAX_PROBE
    # probe select
    assert all(T.ivf_select_trips(nlist, nlist) == (1, 1) and T.ivf_centroid_slices(nq, nlist) == [T.ceil_div(nlist, 32)]
               for nlist in T.IVF_EXISTING_NLIST for nq in (1, T.IVF_EXISTING_MAX_NQ))
    probes = T.IVF_PROBE_CASES + T.IVF_PROBE_PASS_CASES
    assert {(nlist, nprobe) for nlist, nprobe, _, _ in T.IVF_PROBE_CASES} == {(257, 1), (257, 256), (257, 257), (1024, 257), (1024, 1000), (1024, 1024),
                                                                              (1500, 1), (1500, 256), (1500, 1000), (1500, 1024)}
    for pair in {c[:2] for c in T.IVF_PROBE_CASES}:
        assert {nq for nlist, nprobe, nq, _ in T.IVF_PROBE_CASES if (nlist, nprobe) == pair} == {1, 33}
    assert all(nprobe <= nlist for nlist, nprobe, _, _ in probes) and {d for _, _, _, d in probes} == set(T.IVF_TYPES)
    _has("dense_ivf.hip", "three chunks of the tie loop", any(T.ivf_select_trips(nlist, nprobe)[0] >= 3 for nlist, nprobe, _, _ in probes))
    _has("dense_ivf.hip", "two trips of the ranking loop", any(T.ivf_select_trips(nlist, nprobe)[1] >= 2 for nlist, nprobe, _, _ in probes))
    _has("dense_ivf.hip", "an LDS list of exactly IVF_MAX_PROBE entries", any(min(nlist, nprobe) == 1024 for nlist, nprobe, _, _ in probes))
    spread = 0
    for nlist, nprobe in sorted({c[:2] for c in T.IVF_PROBE_CASES}):
        row = T.ivf_crafted_scores(nlist)
        assert set(row) == {-1, 0, 1} and all(set(row[c0: c0 + 200]) == {-1, 0, 1} for c0 in range(0, nlist - 200, 256))
        value, need, ties, taken = T.ivf_select_ties(row, nprobe)
        assert sum(taken) == need and len(ties) == T.ivf_select_trips(nlist, nprobe)[0]
        # ties at T in several chunks, the winners among them in several chunks, and not all of them win
        spread += sum(1 for t in ties if t) >= 2 and sum(1 for t in taken if t) >= 2 and need < sum(ties) and taken[-1] < ties[-1]
    _has("dense_ivf.hip", "keys equal to T in at least two chunks, the lowest lists of them taken across chunks", spread >= 2)
    # centroid-score slices
    slices = [T.ivf_centroid_slices(min(nq, T.PASS), nlist) for nlist, _, nq, _ in probes]
    _has("dense_ivf.hip", "centroid tiles split unevenly over blockIdx.y", any(len(s) >= 2 and len(set(s)) > 1 for s in slices))
    assert [9 * (y + 1) // 2 - 9 * y // 2 for y in range(2)] == T.ivf_centroid_slices(1, 257) == [4, 5] and len(T.ivf_centroid_slices(33, 1500)) == 11
    # update rounds
    assert max(T.ivf_update_rounds(m)[0] for m in T.IVF_EXISTING_UPDATE_LENS) == 1 and set(T.IVF_EXISTING_UPDATE_LENS) < set(T.IVF_UPDATE_LENS)
    _has("dense_ivf.hip", "three update rounds, the last one ragged",
         any(T.ivf_update_rounds(m)[0] >= 3 and T.ivf_update_rounds(m)[1] < 4 and m % 256 for m in T.IVF_UPDATE_LENS))
    assert {1023, 1024, 1025, 2305} <= set(T.IVF_UPDATE_LENS) and T.ivf_update_rounds(2305) == (3, 2) and T.ivf_update_rounds(1025) == (2, 1)
    assert [d for (d,) in T.IVF_UPDATE_CASES] == [1, 64, 65, 200]
    # rank trips, scan slices and the pass loop of the search
    assert T.ivf_rank_trips(T.IVF_EXISTING_MAX_LIST) == 1
    _has("dense_ivf.hip", "a second trip of the rank fold", max(T.ivf_rank_trips(s) for s in T.IVF_SEARCH_SIZES) >= 2)
    assert max(T.IVF_SEARCH_SIZES) > 2048 and {0, 1, 31, 32, 33} <= set(T.IVF_SEARCH_SIZES)
    nlist, tiles = len(T.IVF_SEARCH_SIZES), max(T.ceil_div(s, 32) for s in T.IVF_SEARCH_SIZES)
    searches = T.IVF_SEARCH_CASES + T.IVF_SEARCH_PASS_CASES
    for dtype in T.IVF_TYPES:
        mine = [c[1:] for c in T.IVF_SEARCH_CASES if c[0] == dtype]
        assert {nq for nq, _, _ in mine} == {1, 33} and {k for _, _, k in mine} == {1, 10, 1024} and {1, nlist} <= {p for _, p, _ in mine}
    assert any(T.ivf_scan_slices(nq, nprobe, nlist) > 1 for _, nq, nprobe, _ in searches)
    assert T.ivf_passes(T.IVF_EXISTING_MAX_NQ, T.ivf_plan(T.IVF_EXISTING_MAX_NQ, 130, 130, 5)[0]) == 1
    _has("dense_ivf.hip", "a second pass of srx_ivf_search", any(T.ivf_passes(nq, T.ivf_plan(nq, nlist, nprobe, tiles)[0]) >= 2 for _, nq, nprobe, _ in searches))
    _has("dense_ivf.hip", "a second pass of srx_ivf_probe", any(T.ceil_div(nq, T.PASS) >= 2 for _, _, nq, _ in probes))
    assert all(T.ivf_workspace_bytes(nq, nlist, nprobe, k, tiles) < 64 * MB for _, nq, nprobe, k in searches)  # tens of MB at most


# ---- dense_ivfpq.hip ------------------------------------------------------------------------------------------------------------
IVFPQ_SEARCHES = T.IVFPQ_INSTANCE_CASES + [c[:3] for c in T.IVFPQ_DEEP_CASES + T.IVFPQ_PASS_CASES + T.IVFPQ_SCORER_CASES] + [(4, 16, "f16")]


def test_ivfpq_scan_and_encoder_instances():
    src = _src("dense_ivfpq.hip")
    _quoted(src, "constexpr int ivfpq_scan_threads(int np) { return np <= 2 ? 256 : (np == 6 || np == 7) ? 1024 : 512; }",
            "inline int ivfpq_pieces(int M) { return (M + 15) / 16; }", "switch (ivfpq_pieces(a.M)) {")
    parsed = _macro_args(src, "SRX_IVFPQ")
    assert len(parsed) == len(set(parsed))
    old = {_np(dsub, dim) for dsub, dim, _ in T.IVFPQ_EXISTING}
    new = {_np(dsub, dim) for dsub, dim, _ in T.IVFPQ_INSTANCE_CASES}
    _unreached("dense_ivfpq.hip", "srx_ivfpq_scan_kernel NP", parsed, old | new)
    assert old == {1, 2, 4, 6} and new == {3, 5, 7, 8}
    assert {T.ivfpq_scan_threads(np_) for np_ in new} == {512, 1024} and {T.ivfpq_scan_threads(np_) for np_ in old} == {256, 512, 1024}
    # the encoder's switch runs once per index type; the scorer's once
    launches = _dsub_launches(src)
    assert {k for k, _ in launches} == {"srx_ivfpq_encode_kernel", "srx_ivfpq_score_docs_kernel"}
    types = [TYPE_NAMES[t] for t in re.findall(r"ivfpq_launch_encode<(SRX_HALF_\w+)>\(a, dsub", src)]
    assert sorted(types) == ["bf16", "f16"]
    parsed = {(dsub, t) for k, dsub in launches if k == "srx_ivfpq_encode_kernel" for t in types}
    old = {(dsub, dtype) for dsub, _, dtype in T.IVFPQ_EXISTING}
    _unreached("dense_ivfpq.hip", "srx_ivfpq_encode_kernel (DSUB, TYPE)", parsed, old | {(dsub, dtype) for dsub, _, dtype in IVFPQ_SEARCHES})
    assert parsed - old == {(16, "f16"), (4, "bf16")} <= {(dsub, dtype) for dsub, _, dtype in T.IVFPQ_INSTANCE_CASES}
    scorer = {dsub for dsub, _, _ in T.IVFPQ_EXISTING[:4] + T.IVFPQ_INSTANCE_CASES}  # test_bit_for_bit and the cases that run it
    _unreached("dense_ivfpq.hip", "srx_ivfpq_score_docs_kernel DSUB", {dsub for k, dsub in launches if k == "srx_ivfpq_score_docs_kernel"}, scorer)


def test_ivfpq_loop_shapes():
    src = _src("dense_ivfpq.hip")
    _quoted(src, "const int64_t T = (int64_t)nprobe * max_list_tiles;", "int64_t qb = (1ll << 30) / (256 * T);", "int64_t s = 512 / (p.P > 0 ? p.P : 1);",
            "if (s > 64) s = 64;", "if (s > (T + 15) / 16) s = (T + 15) / 16;", "p.L = (T + p.S - 1) / p.S;", "const int per = (total + S - 1) / S;",
            "int g = g0 + wave;", "const int ng = g + NW;", "for (int64_t c0 = 0; c0 < cols; c0 += THREADS * IVFPQ_NPT) {",
            "for (int q0 = 0; q0 < nq; q0 += pl.P) {", "for (int j = tid; j < a.nprobe; j += THREADS) {",
            "if (4 * tid < a.nprobe && 4 * tid + 4 >= a.nprobe) pre[a.nprobe] = s;", "constexpr int IVFPQ_DOCS_CHUNK = 8 * IVFPQ_DOCS_THREADS;")
    assert _capi.SRX_IVFPQ_PASS == T.PASS
    # what ran so far: the deepest walk is two steps, the widest slice 384 columns, one pass, several slices
    sizes, dsub, nq, nprobe = T.IVFPQ_EXISTING_SLICED
    tiles = T.ivfpq_list_tiles(sizes)
    P, S, L = T.ivfpq_plan(nq, len(sizes), nprobe, max(tiles))
    old = T.ivfpq_walks(sizes, range(len(sizes)), S, 1)
    assert (P, S, L) == (1, 8, 16) and max(max(w) for w, _, _ in old) == 2 and max(T.ivfpq_rank_trips(cols) for _, _, cols in old) == 1
    nlist, big = len(T.IVFPQ_SIZES), max(T.ivfpq_list_tiles(T.IVFPQ_SIZES))
    assert T.ivfpq_plan(T.IVFPQ_EXISTING_MAX_NQ, nlist, nlist, big)[:2] == (33, 2)  # never one slice that is the whole concatenation
    # the deep walks
    tiles = T.ivfpq_list_tiles(T.IVFPQ_DEEP_SIZES)
    assert 0 in tiles and 1 in tiles and sorted(tiles)[-2:] == [25, 25]
    deep = {}
    for dsub, dim, dtype, nq in T.IVFPQ_DEEP_CASES:
        np_, n = _np(dsub, dim), len(T.IVFPQ_DEEP_SIZES)
        P, S, L = T.ivfpq_plan(nq, n, n, max(tiles))
        assert nq > 512 and (P, S, L) == (nq, 1, n * max(tiles)) and T.ivfpq_workspace_bytes(nq, n, n, 1024, T.subspaces(dim, dsub), max(tiles)) < 100 * MB
        for order in (list(range(n)), list(range(n))[::-1], [4, 0, 2, 3, 1]):  # whatever order the probe gives the lists
            (walk, crossed, cols), = T.ivfpq_walks(T.IVFPQ_DEEP_SIZES, order, S, np_)
            assert min(walk) >= 3 and T.deep([walk]) and crossed >= 1 and len(walk) == T.ivfpq_scan_threads(np_) // 64, (np_, order, walk)
            assert cols == sum(tiles) * 64 > 2048 and T.ivfpq_rank_trips(cols) >= 3
        deep[np_] = len(walk)
    assert deep == {7: 16, 8: 8, 1: 4}  # NP -> waves
    # the pass loop
    _has("dense_ivfpq.hip", "a second pass", any(T.ceil_div(nq, T.ivfpq_plan(nq, nlist, nprobe, big)[0]) >= 2 for _, _, _, nq, nprobe in T.IVFPQ_PASS_CASES))
    assert T.ceil_div(T.IVFPQ_EXISTING_MAX_NQ, T.ivfpq_plan(T.IVFPQ_EXISTING_MAX_NQ, nlist, nlist, big)[0]) == 1
    # the prepare kernel
    assert T.ivfpq_prepare(T.IVFPQ_EXISTING_MAX_NPROBE) == (1, 2, 1)
    prep = {nprobe: T.ivfpq_prepare(nprobe) for (nprobe,) in T.IVFPQ_PREPARE_CASES}
    assert prep == {255: (1, 64, 63), 257: (2, 65, 64), 1023: (4, 256, 255), 1024: (4, 256, 255)}
    sizes = T.ivfpq_prepare_sizes()
    assert len(sizes) == T.IVFPQ_PREPARE_NLIST >= max(prep) and sum(sizes) >= len(sizes) and {0, 1, 2, 65} == set(sizes)
    assert all(T.ivfpq_workspace_bytes(3, len(sizes), nprobe, 1024, 4, 2) < 16 * MB for nprobe in prep)
    # the scorer of given docs
    assert {T.scorer_grid(m) for m in T.IVFPQ_EXISTING_SCORER_M} == {(1, 1)}
    assert {T.scorer_grid(m) for _, _, _, m in T.IVFPQ_SCORER_CASES} == {(1, 2), (2, 5)}


# ---- the restated plans against the package's own formulas and the library ------------------------------------------------------
def _around(*values):
    return sorted({max(1, v + d) for v in values for d in (-1, 0, 1)})


def test_restated_plans_agree_with_the_package_and_the_library():
    L = _capi.lib()
    # PQ: (QB, ns, bytes)
    shapes = {(nq, n, T.subspaces(dim, dsub)) for dsub, dim, n, nq in T.PQ_DEEP_CASES + T.PQ_PASS_CASES + T.PQ_EXISTING}
    shapes |= {(33, n, T.subspaces(dim, dsub)) for dsub, dim, n in T.PQ_INSTANCE_CASES}
    for nq, n, M in sorted(shapes):
        for nq_ in _around(nq, T.PASS):
            for n_ in _around(n, 16384):
                for k in (1, 10, 1024):
                    QB, qb, ld, ns = T.half_plan(nq_, n_, k)
                    want = (QB, ns, T.pq_workspace_bytes(nq_, n_, M, k))
                    assert pq.search_plan(nq_, n_, M, k) == want, (nq_, n_, M, k)
                    assert L.srx_pq_workspace_bytes(nq_, n_, M, k) == want[2], (nq_, n_, M, k)
    assert T.half_plan(70, 40_000, 10)[3] == 2 and T.half_plan(5000, 1 << 26, 10)[0] == 32
    # IVF: the bytes hold P
    tiles = max(T.ceil_div(s, 32) for s in T.IVF_SEARCH_SIZES)
    shapes = {(nq, len(T.IVF_SEARCH_SIZES), nprobe, k, tiles) for _, nq, nprobe, k in T.IVF_SEARCH_CASES + T.IVF_SEARCH_PASS_CASES}
    shapes |= {(nq, nlist, nprobe, 1, 1) for nlist, nprobe, nq, _ in T.IVF_PROBE_CASES + T.IVF_PROBE_PASS_CASES}
    shapes |= {(129, 130, 130, 1024, 5), (5000, 65536, 1024, 100, 300), (7, 4000, 64, 10, 1 << 20)}  # a memory-bound P
    for nq, nlist, nprobe, k, t in sorted(shapes):
        for nq_ in _around(nq):
            for t_ in _around(t):
                want = T.ivf_workspace_bytes(nq_, nlist, nprobe, k, t_)
                assert ivf.workspace_bytes(nq_, nlist, nprobe, k, t_) == want, (nq_, nlist, nprobe, k, t_)
                assert L.srx_ivf_workspace_bytes(nq_, nlist, nprobe, k, t_) == want, (nq_, nlist, nprobe, k, t_)
    assert T.ivf_plan(7, 4000, 64, 1 << 20)[0] == 1 and T.ivf_plan(5000, 65536, 1024, 300)[0] == 27
    # IVF-PQ: (P, S, L, bytes)
    shapes = set()
    for sizes, cases in ((T.IVFPQ_DEEP_SIZES, [(dsub, dim, nq, len(T.IVFPQ_DEEP_SIZES)) for dsub, dim, _, nq in T.IVFPQ_DEEP_CASES]),
                         (T.IVFPQ_SIZES, [(dsub, dim, nq, nprobe) for dsub, dim, _, nq, nprobe in T.IVFPQ_PASS_CASES]),
                         (T.IVFPQ_SIZES, [(dsub, dim, 33, 3) for dsub, dim, _ in T.IVFPQ_INSTANCE_CASES]),
                         (T.ivfpq_prepare_sizes(), [(4, 16, 3, nprobe) for (nprobe,) in T.IVFPQ_PREPARE_CASES])):
        shapes |= {(nq, len(sizes), nprobe, T.subspaces(dim, dsub), max(T.ivfpq_list_tiles(sizes))) for dsub, dim, nq, nprobe in cases}
    shapes |= {(1, 3, 3, 2, 41), (5000, 65536, 1024, 128, 1 << 15), (5000, 4000, 64, 96, 300)}  # nprobe * tiles <= 2^26
    for nq, nlist, nprobe, M, t in sorted(shapes):
        for nq_ in _around(nq, 512):
            for t_ in _around(t):
                for k in (1, 10, 1024):
                    want = T.ivfpq_plan(nq_, nlist, nprobe, t_) + (T.ivfpq_workspace_bytes(nq_, nlist, nprobe, k, M, t_),)
                    assert ivfpq.search_plan(nq_, nlist, nprobe, k, M, t_) == want, (nq_, nlist, nprobe, k, M, t_)
                    assert L.srx_ivfpq_workspace_bytes(nq_, nlist, nprobe, k, M, t_) == want[3], (nq_, nlist, nprobe, k, M, t_)


# ---- the table itself -----------------------------------------------------------------------------------------------------------
def test_the_case_lists_are_plain_tuples_without_duplicates():
    lists = {name: getattr(T, name) for name in dir(T) if name.endswith("_CASES")}
    # a case taken out of the table fails here, whatever the loop-shape assertions above still find
    assert {name: len(cases) for name, cases in lists.items()} == {
        "PQ_INSTANCE_CASES": 8, "PQ_DEEP_CASES": 2, "PQ_PASS_CASES": 1, "PQ_SCORER_CASES": 2,
        "IVF_PROBE_CASES": 20, "IVF_PROBE_PASS_CASES": 1, "IVF_SEARCH_CASES": 10, "IVF_SEARCH_PASS_CASES": 1, "IVF_ASSIGN_CASES": 10, "IVF_UPDATE_CASES": 4,
        "IVFPQ_INSTANCE_CASES": 4, "IVFPQ_DEEP_CASES": 3, "IVFPQ_PASS_CASES": 1, "IVFPQ_PREPARE_CASES": 4, "IVFPQ_SCORER_CASES": 2}
    for cases in lists.values():
        assert all(type(c) is tuple for c in cases) and len(set(cases)) == len(cases)
        assert all(type(x) in (int, str) for c in cases for x in c)
