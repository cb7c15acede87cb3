"""The arithmetic of tests/dense_scale.py with Python integers, and the widths of the ctypes table against the headers.

The table: every case crosses the boundary it is named for, plants rows on both sides of it in every layout it stores, and
stays under the device-memory cap; the three plan sizes have the QB they are written for.

The ABI: every prototype of the seventeen headers is parsed (comments stripped; each argument and the return type classified
as pointer / int32 / int64 / float / double / void) and compared with the ``*_SYMBOLS`` entry of the same name, so an
``int64_t n_docs``, ``ld``, ``row0`` or ``workspace_bytes`` bound as ``c_int32`` -- harmless below 2^31, wrong at the sizes of
dense_scale.py -- fails here.  The three structs the other CPU tests do not pin are laid out from the header's field order
with natural alignment and compared with ctypes' offsets."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dense_scale as T  # noqa: E402
import parity  # noqa: E402
from sparse_rx import _capi  # noqa: E402

ALL = T.CASES + T.PLAN_CASES


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_crosses_its_boundaries(case):
    assert case.boundaries or case.matrix or case.qb, f"{case.name}: written for nothing"
    for name in case.boundaries:
        B = case.boundary_bytes(name)
        for per, ub in case.units():
            last_unit_start = (case.n_docs - 1) // per * ub
            assert last_unit_start >= B, f"{case.name}: the last row starts at byte {last_unit_start}, below {name} = {B}"
            if name.startswith("E"):  # the element index of the last row's first element, as row * dim
                per_elem = ub // T.ELEM[case.kind]
                assert (case.n_docs - 1) // per * per_elem >= {"E31": T.E31, "E32": T.E32}[name], (case.name, name)
    for name in case.matrix:
        cells = T.matrix_cells(case, name)
        assert cells, f"{case.name}: {name} falls into no row of the pass's score matrix"
        M = {"MB32": T.B32 // 4, "ME31": T.E31}[name]
        assert T.matrix_last_cell(case) >= M, (case.name, name, T.matrix_last_cell(case))
        for q, d in cells:
            assert q * T.pad64(case.n_docs) + d == M and {d - 1, d} <= set(case.planted()), (case.name, name, q, d)
    assert case.n_docs % 32 and case.n_docs % 64, f"{case.name}: no partial last tile"
    assert 0 <= case.doc_base_top and case.doc_base_top + case.n_docs == (1 << 31) - 2


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_plants_rows_on_both_sides(case):
    rows = case.planted()
    assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == case.n_docs - 1
    for t in (32, 64):
        in_last = [r for r in rows if r >= case.n_docs // t * t]
        assert len(in_last) >= 3, f"{case.name}: {len(in_last)} planted rows in the last partial tile of {t}"
    for name in case.boundaries:
        B = case.boundary_bytes(name)
        for (per, ub), (lo, hi) in zip(case.units(), case.sides(name)):
            assert lo and hi, f"{case.name}: {name} has planted rows {len(lo)} below / {len(hi)} above in the layout of {per}-row units"
            assert max(lo) // per == B // ub - 1, f"{case.name}: the last unit at or below {name} is not planted"
            assert -(-B // ub) in {r // per for r in hi}, f"{case.name}: the first unit at or above {name} is not planted"
            if B % ub:
                assert B // ub in {r // per for r in rows}, f"{case.name}: the unit that straddles {name} is not planted"
    if case.kind == "binary":  # no > 0 rule: the zero rows tie at one distance and fill the tail of the m nearest
        assert len(rows) < case.k, f"{case.name}: the tail of the {case.k} nearest must reach the background"
    else:
        assert len(rows) > case.k, f"{case.name}: a query that ranks every planted row must have more than k = {case.k} of them"


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_stays_under_the_cap(case):
    assert case.device_bytes() <= T.ARENA_BYTES <= T.CAP_BYTES, (case.name, case.device_bytes(), T.ARENA_BYTES)


def test_only_one_case_above_8_gib_plus_workspace():
    big = [c.name for c in T.CASES if c.corpus_bytes() > (9 << 30)]
    assert big == ["b-f32-1024"], big


@pytest.mark.parametrize("case", T.PLAN_CASES, ids=[c.name for c in T.PLAN_CASES])
def test_plan_cases_have_their_qb(case):
    p = parity.dense_plan(case.nq, case.n_docs, case.k, case.dim)
    assert p["QB"] == case.qb and p["passes"] == 2 and case.nq == case.qb + 1, (case.name, p)
    assert parity.dense_qb(case.n_docs) == case.qb
    ws = parity.dense_ws(case.nq, case.n_docs, case.k)
    if "MB32" in case.matrix:
        assert ws["qb"] * T.pad64(case.n_docs) * 4 > T.B32
    if "ME31" in case.matrix:
        assert (ws["qb"] - 1) * T.pad64(case.n_docs) >= T.E31, "q * ld alone must leave int32 in the last row of the pass"


def test_plan_sizes_of_the_issue():
    got = {parity.dense_plan(q + 1, n, 10, 32)["QB"] for n, q in ((1_100_013, 960), (4_000_013, 256), ((1 << 25) + 77, 32))}
    assert got == {960, 256, 32}
    assert [c.qb for c in T.PLAN_CASES] == [960, 256, 32, 32]


@pytest.mark.parametrize("conv", T.CONVERT_CASES, ids=[f"{c[1]}-{c[2]}" for c in T.CONVERT_CASES])
def test_convert_chunks_lie_across_byte_2_32(conv):
    entry, kind, dim, tile, n_rows = conv
    row0, n_total, row_bytes, lo, hi = T.convert_geometry(kind, dim, tile, n_rows)
    assert lo < T.B32 < hi, (conv, lo, hi)
    assert row0 % max(tile, 32) == 0 and row0 + n_rows <= n_total
    guard = T.CONVERT_GUARD_TILES * max(tile, 1) * row_bytes
    assert lo - guard >= 0 and hi + guard <= n_total * row_bytes <= T.ARENA_BYTES


def test_filter_case_bit_index_past_2_32():
    n, rows = T.FILTER_CASE["n_docs"], T.FILTER_CASE["n_filters"]
    w = T.filter_words(n)
    assert w % 4 == 0 and w * 32 >= n > (w - 4) * 32
    assert (rows - 1) * w * 32 >= 1 << 32 and (rows - 2) * w * 32 < 1 << 32, "the last row, and only it, starts past bit 2^32"
    assert rows * w * 4 <= T.ARENA_BYTES


# ---- the ABI --------------------------------------------------------------------------------------------------------------
HEADERS = ["sparse_rx.h", "sparse_rx_rescore.h", "sparse_rx_quant.h", "sparse_rx_filter.h", "sparse_rx_half.h", "sparse_rx_mmr.h",
           "sparse_rx_terms.h", "sparse_rx_maxsim.h", "sparse_rx_fields.h", "sparse_rx_collapse.h", "sparse_rx_facets.h",
           "ext/sparse_rx_feedback.h", "order/sparse_rx_order.h", "boost/sparse_rx_boost.h", "ltr/sparse_rx_ltr.h", "eval/sparse_rx_eval.h",
           "binary/sparse_rx_binary.h"]
TABLES = ["SYMBOLS", "RESCORE_SYMBOLS", "QUANT_SYMBOLS", "FILTER_SYMBOLS", "HALF_SYMBOLS", "MMR_SYMBOLS", "TERMS_SYMBOLS", "MAXSIM_SYMBOLS",
          "FIELDS_SYMBOLS", "COLLAPSE_SYMBOLS", "FACET_SYMBOLS", "FEEDBACK_SYMBOLS", "ORDER_SYMBOLS", "BOOST_SYMBOLS", "LTR_SYMBOLS",
          "EVAL_SYMBOLS", "BINARY_SYMBOLS"]
N_PROTOTYPES = 83

_SCALARS = {"int": "int32", "int32_t": "int32", "uint32_t": "int32", "int64_t": "int64", "float": "float", "double": "double", "void": "void"}


def _strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^\s*#.*$", " ", text, flags=re.M)


def _classify(decl):
    """one C parameter or return type -> pointer / int32 / int64 / float / double / void"""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in re.findall(r"[A-Za-z_]\w*", decl) if w not in ("const", "unsigned", "signed", "struct", "enum")]
    assert words, decl
    for w in words:  # the type is the first word that names one; what follows is the parameter's name
        if w in _SCALARS:
            return _SCALARS[w]
    raise AssertionError(f"unknown C type in {decl!r}")


def _prototypes(header):
    """{name: (return class, [argument classes])} of one header"""
    text = _strip(open(os.path.join(ROOT, "include", header), encoding="utf-8").read())
    text = re.sub(r"typedef\s+(struct|enum)\b[^{;]*\{.*?\}[^;]*;", " ", text, flags=re.S)  # the struct and enum bodies
    text = re.sub(r"typedef\s[^;{]*;", " ", text)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(srx_\w+)\s*\(([^()]*)\)\s*;", text):
        args = [a.strip() for a in args.split(",")]
        arg_classes = [] if args == ["void"] or args == [""] else [_classify(a) for a in args]
        assert name not in out, f"{header}: {name} declared twice"
        out[name] = (_classify(ret), arg_classes)
    return out


def _ctype_class(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type(ctypes.POINTER(ctypes.c_int))) and issubclass(t, ctypes._Pointer):
        return "pointer"
    if issubclass(t, ctypes._SimpleCData):
        code, size = t._type_, ctypes.sizeof(t)
        if code in "fd":
            return {"f": "float", "d": "double"}[code]
        if code in "bhilqBHILQ" and size in (4, 8):
            return {4: "int32", 8: "int64"}[size]
    raise AssertionError(f"unclassified ctypes type {t!r}")


def abi_mismatches(tables=None):
    """every disagreement between the headers and the ctypes tables, as text; [] when they agree"""
    problems, seen = [], 0
    for header, table_name in zip(HEADERS, TABLES):
        table = (tables or {}).get(table_name, getattr(_capi, table_name))
        protos = _prototypes(header)
        seen += len(protos)
        for name in sorted(set(protos) ^ set(table)):
            problems.append(f"{header}: {name} is {'declared but not bound' if name in protos else 'bound but not declared'} ({table_name})")
        for name in sorted(set(protos) & set(table)):
            res, args = table[name]
            got = (_ctype_class(res), [_ctype_class(a) for a in args])
            if got != protos[name]:
                want_r, want_a = protos[name]
                where = "return" if got[0] != want_r else next((f"argument {i}" for i, (g, w) in enumerate(zip(got[1], want_a)) if g != w),
                                                               f"argument count {len(got[1])} != {len(want_a)}")
                problems.append(f"{header}: {name}: {where}: header {protos[name]}, {table_name} {got}")
    if seen != N_PROTOTYPES:
        problems.append(f"{seen} prototypes parsed, {N_PROTOTYPES} expected")
    return problems


def test_ctypes_widths_match_the_headers():
    assert len(HEADERS) == len(TABLES) == 17
    assert sum(len(getattr(_capi, t)) for t in TABLES) == N_PROTOTYPES
    problems = abi_mismatches()
    assert not problems, "\n".join(problems)


def test_ctypes_struct_pointers_and_handles_are_pointers():
    p = _prototypes("sparse_rx.h")
    assert p["srx_index_create"] == ("int32", ["pointer", "pointer"]) and p["srx_index_destroy"] == ("void", ["pointer"])
    assert p["srx_last_error"] == ("pointer", []) and p["srx_search_workspace_bytes"] == ("int64", ["pointer", "int32", "int32"])
    assert p["srx_dense_search_f32"][1][-1] == "float" and p["srx_build_impacts"][1][5:8] == ["double"] * 3


@pytest.mark.parametrize("table,name,arg", [("SYMBOLS", "srx_dense_search_i8", 3), ("RESCORE_SYMBOLS", "srx_dense_score_docs_f32", 2),
                                            ("QUANT_SYMBOLS", "srx_dense_quantize_i8", 6), ("FILTER_SYMBOLS", "srx_filter_set_docs", 5),
                                            ("HALF_SYMBOLS", "srx_dense_search_half", 14), ("MAXSIM_SYMBOLS", "srx_maxsim_rerank_half", 3),
                                            ("BINARY_SYMBOLS", "srx_binary_encode", 6), ("SYMBOLS", "srx_dense_workspace_bytes", -1)])
def test_the_abi_check_sees_a_narrowed_or_swapped_argument(table, name, arg):
    """The check itself, on a copy of one table per header family: an int64 narrowed to int32 and two arguments of different
    classes swapped are both reported, under the prototype's name."""
    orig = getattr(_capi, table)
    res, args = orig[name]
    if arg < 0:
        bad = (ctypes.c_int32, list(args))
    else:
        assert args[arg] is ctypes.c_int64
        bad = (res, [ctypes.c_int32 if i == arg else a for i, a in enumerate(args)])
    problems = abi_mismatches({table: {**orig, name: bad}})
    assert len(problems) == 1 and name in problems[0], problems
    if arg >= 0:
        j = next(i for i, a in enumerate(args) if _ctype_class(a) != "int64")
        swapped = list(args)
        swapped[arg], swapped[j] = swapped[j], swapped[arg]
        problems = abi_mismatches({table: {**orig, name: (res, swapped)}})
        assert len(problems) == 1 and name in problems[0], problems


_FIELD_SIZES = {"int32_t": 4, "int64_t": 8, "float": 4, "double": 8}


def _struct_layout(header, struct_name):
    """[(field, offset, size)] and the size of a struct, from the header's field order with natural alignment"""
    text = _strip(open(os.path.join(ROOT, "include", header), encoding="utf-8").read())
    m = re.search(r"typedef\s+struct\s*\w*\s*\{([^}]*)\}\s*" + struct_name + r"\s*;", text, flags=re.S)
    assert m, f"{struct_name} not found in {header}"
    off, align, fields = 0, 1, []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        name = re.findall(r"\w+", decl)[-1]
        size = 8 if "*" in decl else _FIELD_SIZES[next(w for w in re.findall(r"\w+", decl) if w in _FIELD_SIZES)]
        off = -(-off // size) * size
        fields.append((name, off, size))
        off += size
        align = max(align, size)
    return fields, -(-off // align) * align


@pytest.mark.parametrize("header,struct_name,cls", [("sparse_rx.h", "srx_index_desc", "IndexDesc"), ("sparse_rx.h", "srx_search_opts", "SearchOpts"),
                                                    ("sparse_rx_filter.h", "srx_doc_filter", "DocFilterDesc")])
def test_struct_layouts_match_the_headers(header, struct_name, cls):
    fields, size = _struct_layout(header, struct_name)
    c = getattr(_capi, cls)
    assert [f[0] for f in c._fields_] == [f[0] for f in fields], (struct_name, [f[0] for f in c._fields_])
    for name, off, nbytes in fields:
        d = getattr(c, name)
        assert (d.offset, d.size) == (off, nbytes), f"{struct_name}.{name}: ctypes has offset {d.offset} size {d.size}, the header {off} / {nbytes}"
    assert ctypes.sizeof(c) == size, (struct_name, ctypes.sizeof(c), size)
