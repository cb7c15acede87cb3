"""The inventory of the dense family's kernel instances, without a GPU.  The dispatch lines of the six kernel files are parsed
(SRX_HC, SRX_MS, SRX_BN, SRX_MF, SRX_DS, SRX_DQ, the TPW choice of the half Gram and the glog ladder of the i8 scorer); the
cases of tests/dense_instances.py, together with the shapes the units' own test files run, must reach exactly the parsed sets,
and the table must hold a case in every loop-shape class the kernels have.  An instance added to a dispatch line later fails
here until a case reaches it."""
import os
import re

import dense_instances as T
from sparse_rx import _capi


def _src(name):
    with open(os.path.join(_capi.CSRC_DIR, name), encoding="utf-8") as f:
        return f.read()


def _macro_args(src, macro):
    """The argument tuples of every use of a dispatch macro (its #define has a name, not a number, as argument)."""
    return [tuple(int(x) for x in a.split(",")) for a in re.findall(rf"\b{macro}\((\d+(?:, *\d+)*)\)", src)]


def _const(src, name):
    return int(re.search(rf"constexpr int {name} = (\d+)", src).group(1))


def _unreached(unit, what, parsed, reached):
    """Both directions: an instance no case reaches, and a case whose instance the source no longer has."""
    parsed, reached = set(parsed), set(reached)
    assert parsed, f"{unit}: no {what} instance found in the source: the dispatch line has changed, update the parser"
    missing, gone = sorted(parsed - reached, key=repr), sorted(reached - parsed, key=repr)
    assert not missing, f"{unit}: no case of tests/dense_instances.py and no existing test reaches {what} {missing}"
    assert not gone, f"{unit}: the table reaches {what} {gone}, which the dispatch line does not instantiate"


def _has(unit, shape, found):
    assert found, f"{unit}: tests/dense_instances.py holds no case for the loop shape '{shape}'"


# ---- dense_half.hip -------------------------------------------------------------------------------------------------------------
def test_half_convert_instances_and_gemm_loop_shapes():
    src, common = _src("dense_half.hip"), _src("half_common.h")
    assert "const int nj = (a.dim_pad + 255) / 256;" in src and "ld % 4 == 0 && dim % 4 == 0" in src
    assert _const(src, "HG_KB") == T.HALF_KB and _const(common, "HF_QTILE") == T.HALF_QTILE and "q > 1024 ? 1024 : q" in common
    assert "const int n_stages = ks / HG_KB;" in src and "q_filter[q0 + q]" in src
    parsed = {(nj[0], vec) for nj in _macro_args(src, "SRX_HC") for vec in (True, False)}  # the macro launches both load forms
    assert "srx_dense_half_convert_kernel<NJ, true, TYPE>" in src and "srx_dense_half_convert_kernel<NJ, false, TYPE>" in src
    reached = {T.half_convert_instance(dim) for dim, _ in T.HALF_CONVERT_CASES}
    reached |= {T.half_convert_instance(dim, ld, aligned) for dim, ld, aligned in T.HALF_EXISTING_CONVERT}
    _unreached("dense_half.hip", "srx_dense_half_convert_kernel (NJ, VEC)", parsed, reached)
    # every (NJ = 2, load form) is compared byte for byte by the table itself
    assert {(2, True), (2, False)} <= {T.half_convert_instance(dim) for dim, _ in T.HALF_CONVERT_CASES}
    stages = {T.half_n_stages(dim) for _, _, dim, _ in T.HALF_INT_CASES} | {T.half_n_stages(dim) for _, dim in T.HALF_RANDOM_CASES}
    _has("dense_half.hip", "an odd n_stages above 1", any(s > 1 and s % 2 == 1 for s in stages))
    assert {3, 5, 7, 9, 13, 15} <= stages and not stages & {T.half_n_stages(d) for d in T.HALF_EXISTING_SEARCH_DIMS}
    assert all(T.half_n_stages(d) in (1, 2, 4, 12, 16) for d in T.HALF_EXISTING_SEARCH_DIMS)  # even counts and 1: what ran so far
    for n, nq, filtered in T.HALF_EXISTING_FILTERED:  # no existing test has a filtered second pass or query tile
        assert not (filtered and max(T.half_passes(nq, n)) > 1)
    _has("dense_half.hip", "a filtered search of more than one query tile and more than one pass",
         any(T.half_passes(nq, n)[0] > 1 and T.half_passes(nq, n)[1] > 1 for n, _, nq, _, _ in T.HALF_FILTER_CASES))
    for n, dim, nq, k, n_rows in T.HALF_FILTER_CASES:  # the second pass reads other filter rows than the first
        assert T.HALF_PASS % (n_rows + 1) != 0 and nq > T.HALF_PASS


# ---- maxsim.hip -----------------------------------------------------------------------------------------------------------------
def test_maxsim_instances_and_group_loop_shapes():
    src = _src("maxsim.hip")
    assert _const(src, "MS_G") == T.MAXSIM_G and "a.nab = ceil32(tq) / 32;" in src and "gpb = ks / MS_G" in src
    parsed = {a[0] for a in _macro_args(src, "SRX_MS")}
    cases = T.MAXSIM_CASES + [(dim, tq) for dim, tq, _, _ in T.MAXSIM_RERANK_CASES]
    assert all(T.maxsim_shape_ok(tq, dim) for dim, tq in cases + T.MAXSIM_EXISTING)
    _unreached("maxsim.hip", "srx_maxsim_score_kernel NAB", parsed, {T.maxsim_nab(tq) for _, tq in cases + T.MAXSIM_EXISTING})
    assert 3 not in {T.maxsim_nab(tq) for _, tq in T.MAXSIM_EXISTING} and 3 in {T.maxsim_nab(tq) for _, tq in cases}
    _has("maxsim.hip", "an odd gpb above 1", any(T.maxsim_gpb(dim) > 1 and T.maxsim_gpb(dim) % 2 == 1 for dim, _ in cases))
    assert all(T.maxsim_gpb(dim) in (1, 2, 4, 8, 16) for dim, _ in T.MAXSIM_EXISTING)
    # every NAB meets an odd gpb above 1, and NAB = 3 meets gpb = 1 as well
    odd = {T.maxsim_nab(tq) for dim, tq in cases if T.maxsim_gpb(dim) > 1 and T.maxsim_gpb(dim) % 2 == 1}
    assert odd == parsed and (3, 1) in {(T.maxsim_nab(tq), T.maxsim_gpb(dim)) for dim, tq in cases}


# ---- mmr.hip --------------------------------------------------------------------------------------------------------------------
def test_mmr_instances_and_chunk_loop_shapes():
    src = _src("mmr.hip")
    assert _const(src, "MG_PIECES") == T.MMR_PIECES and _const(src, "MG_THREADS") == 64 * T.MMR_WAVES
    assert "const int kc = MG_PIECES / (nb * 64);" in src and "if (a.m <= 128)" in src
    tpw = {int(x) for x in re.findall(r"srx_mmr_gram_half_kernel<TYPE, (\d+)>", src)}
    half = T.MMR_HALF_CASES + T.MMR_HALF_EXACT_CASES
    old = T.MMR_EXISTING + T.MMR_EXISTING_HALF_ONLY
    _unreached("mmr.hip", "srx_mmr_gram_half_kernel TPW", tpw, {T.mmr_half_plan(dim, m)[2] for dim, m in half + old})
    plans = [T.mmr_half_plan(dim, m) for dim, m in half]
    old_plans = [T.mmr_half_plan(dim, m) for dim, m in old]
    nbs = {p[0] for p in plans} | {p[0] for p in old_plans}
    for nb in range(1, 9):
        _has("mmr.hip", f"half Gram nb = {nb}", nb in nbs)
    assert {p[0] for p in old_plans} == {1, 2, 4, 8} and {3, 5, 6, 7} <= {p[0] for p in plans}
    short_last = lambda p: len(p[3]) > 1 and p[3][-1] < p[3][0]
    _has("mmr.hip", "a last K chunk shorter than an earlier one", any(short_last(p) for p in plans))
    assert not any(short_last(p) for p in old_plans)  # every existing pair has ks below kc or divisible by it
    assert [T.mmr_half_plan(200, m)[3] for m in (96, 160, 192)] == [[10, 6], [6, 6, 4], [5, 5, 5, 1]] and T.mmr_half_plan(768, 32)[3] == [32, 16]
    _has("mmr.hip", "TPW = 4 with fewer than 64 tiles", any(p[2] == 4 and p[4] < 4 * T.MMR_WAVES for p in plans))
    assert {p[4] for p in plans if p[2] == 4} == {25, 36, 49} and not any(p[2] == 4 and p[4] < 64 for p in old_plans)
    # the f32 Gram's buckets
    parsed = {a[0] for a in _macro_args(src, "SRX_MF")}
    assert parsed == set(T.MMR_F32_BUCKETS) and "if (ns <= NS)" in src
    f32 = T.MMR_F32_CASES + T.MMR_F32_EXACT_CASES
    _unreached("mmr.hip", "srx_mmr_gram_f32_kernel NS", parsed, {T.mmr_f32_ns(dim)[0] for dim, _ in f32 + T.MMR_EXISTING})
    assert 8 not in {T.mmr_f32_ns(dim)[0] for dim, _ in T.MMR_EXISTING}
    _has("mmr.hip", "an f32 Gram bucket wider than the row", any(T.mmr_f32_ns(dim)[1] for dim, _ in f32))
    assert not any(T.mmr_f32_ns(dim)[1] for dim, _ in T.MMR_EXISTING)
    assert {T.mmr_f32_ns(dim)[0] for dim, _ in f32 if T.mmr_f32_ns(dim)[1]} == {4, 8, 12, 16}  # slack in every bucket that can have it


# ---- dense_binary.hip -----------------------------------------------------------------------------------------------------------
def test_binary_instances_and_query_loop_shapes():
    src = _src("dense_binary.hip")
    assert _const(src, "BN_QTILE") == T.BINARY_QTILE and _const(src, "BN_PASS") == T.BINARY_PASS
    assert "bin_launch_dist(a, W / 4, stream);" in src and "filter->q_filter + q0" in src
    parsed = {a[0] for a in _macro_args(src, "SRX_BN")}
    search = {T.binary_nj(c[0]) for c in T.BINARY_SEARCH_CASES}
    _unreached("dense_binary.hip", "srx_binary_dist_kernel NJ", parsed, search | {T.binary_nj(d) for d in T.BINARY_EXISTING_SEARCH_DIMS})
    assert {T.binary_nj(d) for d in T.BINARY_EXISTING_SEARCH_DIMS} == {1, 2, 8} and {3, 4, 5, 6, 7} <= search
    for nj in (2, 8):  # the two instances that ran already, at a dim below dim_pad
        assert any(T.binary_nj(c[0]) == nj and c[0] % 128 for c in T.BINARY_SEARCH_CASES)
    # the scorer of given docs takes nj at run time: every value the search has an instance for
    _unreached("dense_binary.hip", "srx_binary_dist_docs nj", parsed, {T.binary_nj(d) for (d,) in T.BINARY_DOCS_CASES})
    assert {T.binary_nj(d) for d in T.BINARY_EXISTING_DOCS_DIMS} == {2}
    for n, nq, filtered in T.BINARY_EXISTING_FILTERED:
        assert not (filtered and max(T.binary_passes(nq, n)) > 1)
    _has("dense_binary.hip", "a filtered search of more than one query tile and more than one pass",
         any(T.binary_passes(nq, n)[0] > 1 and T.binary_passes(nq, n)[1] > 1 for n, _, nq, _, _ in T.BINARY_FILTER_CASES))
    for n, dim, nq, m, n_rows in T.BINARY_FILTER_CASES:
        assert T.BINARY_PASS % (n_rows + 1) != 0 and nq > T.BINARY_PASS
        assert n % 64 != 0 and m >= n % 64  # the docs of the last partial tile that a residue row allows are all candidates


# ---- dense_score.hip ------------------------------------------------------------------------------------------------------------
def test_score_instances_and_slack():
    src = _src("dense_score.hip")
    parsed = set(_macro_args(src, "SRX_DS"))
    assert parsed == set(T.SCORE_BUCKETS) and "if (ns <= NS)" in src and "launch_rows<true>" in src and "launch_rows<false>" in src
    for engine in ("f32", "u8"):  # IS_U8 is a template argument: the ladder is instantiated for each
        new = [T.score_rows_instance(dim) for e, dim, _ in T.SCORE_ROWS_CASES if e == engine]
        old = [T.score_rows_instance(dim) for e, dim in T.SCORE_EXISTING_ROWS if e == engine]
        _unreached("dense_score.hip", f"srx_dense_score_rows_kernel ({engine}) (NS, U)", parsed, {b for b, _ in new + old})
        _has("dense_score.hip", f"a bucket wider than the row, {engine}", any(slack for _, slack in new))
        assert (8, 8) not in {b for b, _ in old}
        assert {(b[0], slack) for b, slack in new} == {(4, False), (8, True), (8, False), (16, True)}
    assert not any(T.score_rows_instance(dim)[1] for e, dim in T.SCORE_EXISTING_ROWS if e == "u8")  # u8 never ran with slack
    # the i8 scorer: the ladder glog == 1 / glog == 2 / else, and the row lengths the entry point takes
    ladder = {int(g): int(u) for g, u in re.findall(r"a\.glog == (\d+)\)\s*hipLaunchKernelGGL\(srx_dense_score_i8_kernel<(\d+)>", src)}
    ladder["else"] = int(re.search(r"else\s*hipLaunchKernelGGL\(srx_dense_score_i8_kernel<(\d+)>", src).group(1))
    assert ladder == T.SCORE_I8_LADDER and len(re.findall(r"srx_dense_score_i8_kernel<\d+>", src)) == len(ladder)
    body = src.split("SRX_API int srx_dense_score_docs_i8")[1]
    dims = tuple(int(x) for x in re.search(r"static const int dims\[\] = \{([^}]*)\}", body).group(1).split(","))
    assert dims == T.SCORE_I8_DIMS and "while ((1 << a.glog) < dim / 16) ++a.glog;" in body
    new, old = {d for d, _, _ in T.SCORE_I8_CASES}, set(T.SCORE_EXISTING_I8_DIMS)
    _unreached("dense_score.hip", "srx_dense_score_i8_kernel U", ladder.values(), {T.score_i8_u(d) for d in new | old})
    _unreached("dense_score.hip", "srx_dense_score_i8_kernel glog", {T.score_i8_glog(d) for d in dims}, {T.score_i8_glog(d) for d in new | old})
    assert 5 not in {T.score_i8_glog(d) for d in old} and {T.score_i8_glog(d) for d in new} == {4, 5}
    for packed in (True, False):
        assert {d for d, _, p in T.SCORE_I8_CASES if p is packed} == new


# ---- dense_quant.hip ------------------------------------------------------------------------------------------------------------
def test_quant_instances():
    src = _src("dense_quant.hip")
    assert "const int nj = (a.dim_pad + 255) / 256;" in src and "ld % 4 == 0 && dim % 4 == 0" in src
    assert "srx_dense_quant_kernel<NJ, true, MODE>" in src and "srx_dense_quant_kernel<NJ, false, MODE>" in src
    modes = re.findall(r"case (DQ_\w+): dq_launch<\1>", src) + re.findall(r"default: dq_launch<(DQ_\w+)>", src)
    assert modes == ["DQ_I8_ROW", "DQ_I8_QUERY", "DQ_U8_ROW", "DQ_U8_QUERY"] and len(modes) == len(T.QUANT_MODES)
    dims = tuple(int(x) for x in re.search(r"static const int dims\[\] = \{([^}]*)\}", src).group(1).split(","))
    assert dims == T.QUANT_I8_DIMS
    parsed = {(a[0], vec, mode) for a in _macro_args(src, "SRX_DQ") for vec in (True, False) for mode in T.QUANT_MODES}
    new = set().union(*(T.quant_instances(dim) for dim, _ in T.QUANT_CASES))
    old = set().union(*(T.quant_instances(dim) for dim in T.QUANT_EXISTING_DIMS))
    _unreached("dense_quant.hip", "srx_dense_quant_kernel (NJ, VEC, MODE)", parsed, new | old)
    assert 2 not in {nj for nj, _, _ in old}  # the gap: nothing quantised a row of 257 .. 512 columns on the device
    assert {i for i in parsed if i[0] == 2} == new


# ---- the table itself -----------------------------------------------------------------------------------------------------------
def test_the_case_lists_are_plain_tuples_without_duplicates():
    lists = [getattr(T, name) for name in dir(T) if name.endswith("_CASES")]
    assert len(lists) == 16
    for cases in lists:
        assert cases and all(type(c) is tuple for c in cases) and len(set(cases)) == len(cases)
        assert all(type(x) in (int, str, bool) for c in cases for x in c)
